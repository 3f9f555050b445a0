"""Dual-clip PPO problems with their numpy float64 reference (test infrastructure; used by test_dual_clip_host.py and test_zzzzzzzzzzzzzzzz_dual_clip_gpu.py).

The surrogate (include/mi355_carla.h, mi_ppo_set_dual_clip): with r = pi_theta / pi_old, s = min(r A, clamp(r, 1 - eps, 1 + eps) A) and a constant c > 1,
    s' = (A < 0 and c A > s) ? c A : s
reference() is the whole step loss with s' -- policy, value and entropy terms -- in numpy float64, with the gradients of all 13 variables by a backward pass
written out here (test_dual_clip_host.py checks it against finite differences), and stats_reference() is the statistics pass.

Shapes: those of the value-clip and KL tests -- 2 actions on 67 -> 500 / 300 (the <2> instantiation of the head / loss kernel) and 3 actions on 5 -> 36 / 20 (the
<8> instantiation) -- and one wide case, 2 actions on 131 -> 36 / 20 (mi_ppo_set_wide_inputs); M = 5 (one partial block), 33 (a second block with one sample),
257 (the chunked weight-gradient route).  Parameters and samples are tests/ppo_shape_cases.build's.

Rows are PLANNED, not random.  With eps = 0.2 and c = 3 row i takes entry i mod 14 of PLAN: a target ratio from {0.5, 0.9, 1.1, 1.5, 2.5, 4, 8} and a sign of A,
every pair once.  The ratio is realised through the cached log pi_old: logp_old[m] = float32(logp64[m] - log(target)), logp64 the float64 log pi_theta of the fp32
parameters.  |A| = 0.25 .. 1.  The classes:
    DUAL     A < 0, r in {4, 8}              c A > r A: the constant, no gradient
    NEG_FLOW A < 0, r in {0.9, 1.1, 1.5, 2.5}  s = r A, the gradient flows (above 1 + eps as well: the open side the dual clip bounds)
    NEG_LOW  A < 0, r = 0.5                  s = (1 - eps) A: clipped from below
    POS_LOW  A > 0, r = 0.5                  s = r A flows
    POS_IN   A > 0, r in {0.9, 1.1}          inside the range
    POS_HIGH A > 0, r in {1.5, 2.5, 4, 8}    s = (1 + eps) A: clipped
Six classes do not fit into five rows: PLAN begins with DUAL, NEG_FLOW, NEG_LOW, POS_LOW, POS_HIGH, so M = 5 holds all three classes of A < 0 and the two
one-sided regions of A > 0; POS_IN -- the arithmetic of NEG_FLOW's inside rows -- appears from row 5 on.  Margins: the thresholds are 0.8, 1.2 and 3; the closest
target is 1.1, 8.3 % under 1.2 (0.9 is 12.5 % above 0.8, 2.5 is 16.7 % under 3), so MARGIN = 0.08 of the threshold is what plan_conditions() asserts: an error
of 1e-4 in a ratio is 800 times too small to move a row between classes."""
from collections import OrderedDict

import numpy as np

import ppo_shape_cases as pc

EPS, C = 0.2, 3.0
EPS32 = float(np.float32(EPS))                            # the range as the kernels see it
TARGETS = (0.5, 0.9, 1.1, 1.5, 2.5, 4.0, 8.0)
THRESHOLDS = (1.0 - EPS, 1.0 + EPS, C)
MARGIN, A_MIN = 0.08, 0.1
MS = (5, 33, 257)
HALF_LOG_2PI = 0.918938533204672741780329736406
# name -> (input_dim, num_actions, hidden, seed, perturb, wide_inputs)
SHAPES = OrderedDict([("A2", (67, 2, (500, 300), 2, 0.02, 0)), ("A3", (5, 3, (36, 20), 11, 0.0231, 0)), ("W131", (131, 2, (36, 20), 5, 0.03, 1))])
DUAL, NEG_FLOW, NEG_LOW, POS_LOW, POS_IN, POS_HIGH = range(6)
CLASS_NAMES = ("DUAL", "NEG_FLOW", "NEG_LOW", "POS_LOW", "POS_IN", "POS_HIGH")
PLAN = ((4.0, -1), (1.5, -1), (0.5, -1), (0.5, +1), (1.5, +1), (1.1, +1), (8.0, -1), (0.9, -1), (2.5, -1), (1.1, -1), (0.9, +1), (2.5, +1), (4.0, +1), (8.0, +1))
assert sorted(PLAN) == sorted((t, s) for t in TARGETS for s in (-1, +1))
NAMES = ("policy/dense/kernel", "policy/dense/bias", "policy/dense_1/kernel", "policy/dense_1/bias", "policy/action_mean/kernel", "policy/action_mean/bias",
         "policy/action_logstd", "policy/dense_2/kernel", "policy/dense_2/bias", "policy/dense_3/kernel", "policy/dense_3/bias", "policy/value/kernel",
         "policy/value/bias")
POLICY_NET, VALUE_NET = NAMES[:7], NAMES[7:]


def class_of(r, A, c=C, eps=EPS32):
    """The class of every row from float64 ratios and advantages (the definition, not the plan)."""
    r, A = np.asarray(r, np.float64), np.asarray(A, np.float64)
    s = np.minimum(r * A, np.clip(r, 1.0 - eps, 1.0 + eps) * A)
    neg = A < 0
    dual = neg & (c * A > s)
    return np.select([dual, neg & (r < 1.0 - eps), neg, r < 1.0 - eps, r <= 1.0 + eps], [DUAL, NEG_LOW, NEG_FLOW, POS_LOW, POS_IN], POS_HIGH)


def forward(theta, s, a, low, high, dtype=np.float64):
    """The two networks in `dtype` on fp32 values -> dict of every intermediate the backward pass needs, log pi_theta(a | s) [M] and V [M]."""
    f = lambda k: np.asarray(theta[k], dtype)      # noqa: E731
    x, act = np.asarray(s, dtype), np.asarray(a, dtype)
    lo, hi = np.asarray(low, dtype), np.asarray(high, dtype)
    o = {"x": x}
    o["z1"] = x @ f(NAMES[0]) + f(NAMES[1]); o["h1"] = np.maximum(o["z1"], 0.0)
    o["z2"] = o["h1"] @ f(NAMES[2]) + f(NAMES[3]); o["h2"] = np.maximum(o["z2"], 0.0)
    o["t"] = np.tanh(o["h2"] @ f(NAMES[4]) + f(NAMES[5]))
    o["mean"] = lo + ((o["t"] + 1.0) / 2.0) * (hi - lo)
    ls = f(NAMES[6])
    o["sigma"] = np.exp(ls)
    o["z"] = (act - o["mean"]) / o["sigma"]
    o["logp"] = (-0.5 * o["z"] ** 2 - (HALF_LOG_2PI + ls)).sum(1)
    o["y1"] = x @ f(NAMES[7]) + f(NAMES[8]); o["g1"] = np.maximum(o["y1"], 0.0)
    o["y2"] = o["g1"] @ f(NAMES[9]) + f(NAMES[10]); o["g2"] = np.maximum(o["y2"], 0.0)
    o["v"] = (o["g2"] @ f(NAMES[11]) + f(NAMES[12])).reshape(-1)
    return o


def reference(theta, s, a, R, adv, logp_old, low, high, c=C, eps=EPS32, value_scale=pc.VALUE_SCALE, entropy_scale=pc.ENTROPY_SCALE, grads=True,
              dtype=np.float64):
    """The step loss with the dual-clipped surrogate in `dtype` -> (scalars, the 13 gradients or None, per-sample dict: ratio, surrogate s, s', du [M, A], dv,
    dual-clipped).  dtype np.float32: the same formulas in fp32, the measure of what fp32 arithmetic alone costs (the bf16x3 bound).
    loss = -mean(s') + value_scale mean((V - R)^2) - entropy_scale sum_a (1/2 + log(2 pi)/2 + logstd[a]).  c = inf: the plain loss."""
    f = lambda k: np.asarray(theta[k], dtype)      # noqa: E731
    o = forward(theta, s, a, low, high, dtype)
    M = len(o["logp"])
    A, Rt = np.asarray(adv, dtype), np.asarray(R, dtype)
    lo, hi = np.asarray(low, dtype), np.asarray(high, dtype)
    eps, value_scale, entropy_scale = dtype(eps), dtype(value_scale), dtype(entropy_scale)
    r = np.exp(o["logp"] - np.asarray(logp_old, dtype))
    s1, s2 = r * A, np.clip(r, dtype(1.0) - eps, dtype(1.0) + eps) * A
    sur = np.minimum(s1, s2)
    with np.errstate(invalid="ignore"):
        dual = (A < 0) & (c * A > sur)
    sur_d = np.where(dual, np.where(dual, c, 0.0) * A, sur).astype(dtype)
    ls = f(NAMES[6])
    policy_loss, value_loss = sur_d.mean(), value_scale * ((o["v"] - Rt) ** 2).mean()
    entropy_loss = entropy_scale * (0.5 + HALF_LOG_2PI + ls).sum()
    scal = dict(policy_loss=float(policy_loss), value_loss=float(value_loss), entropy_loss=float(entropy_loss),
                loss=float(-policy_loss + value_loss - entropy_loss), ratio_mean=float(r.mean()))
    dr = np.where((s1 <= s2) & ~dual, A, dtype(0.0))                                         # tf.minimum / tf.maximum: ties keep the gradient on r A
    coef = -(dr * r) / dtype(M)                                                              # d loss / d log pi per sample
    du = coef[:, None] * (o["z"] / o["sigma"]) * (dtype(0.5) * (hi - lo)) * (dtype(1.0) - o["t"] ** 2)
    dv = dtype(2.0) * value_scale * (o["v"] - Rt) / dtype(M)
    per = dict(ratio=r, surrogate=sur, surrogate_dual=sur_d, du=du, dv=dv, dual=dual, logp=o["logp"], value=o["v"])
    if not grads:
        return scal, None, per
    g = OrderedDict()
    g[NAMES[6]] = (coef[:, None] * (o["z"] ** 2 - dtype(1.0))).sum(0) - entropy_scale
    g[NAMES[4]], g[NAMES[5]] = o["h2"].T @ du, du.sum(0)
    d2 = (du @ f(NAMES[4]).T) * (o["z2"] > 0)
    g[NAMES[2]], g[NAMES[3]] = o["h1"].T @ d2, d2.sum(0)
    d1 = (d2 @ f(NAMES[2]).T) * (o["z1"] > 0)
    g[NAMES[0]], g[NAMES[1]] = o["x"].T @ d1, d1.sum(0)
    g[NAMES[11]], g[NAMES[12]] = o["g2"].T @ dv[:, None], np.array([dv.sum()])
    e2 = (dv[:, None] @ f(NAMES[11]).T) * (o["y2"] > 0)
    g[NAMES[9]], g[NAMES[10]] = o["g1"].T @ e2, e2.sum(0)
    e1 = (e2 @ f(NAMES[9]).T) * (o["y1"] > 0)
    g[NAMES[7]], g[NAMES[8]] = o["x"].T @ e1, e1.sum(0)
    return scal, OrderedDict((k, g[k].reshape(np.shape(theta[k]))) for k in NAMES), per


def stats_reference(logp_new, logp_old, adv, rows, c=C, eps=EPS32):
    """mi_ppo_dual_clip_stats in numpy float64 from the fp32 tables -> [count, count(A < 0), count(dual-clipped), sum s', sum s]."""
    lp, lpo, A = (np.asarray(x)[rows].astype(np.float64) for x in (logp_new, logp_old, adv))
    r = np.exp(lp - lpo)
    sur = np.minimum(r * A, np.clip(r, 1.0 - eps, 1.0 + eps) * A)
    dual = (A < 0) & (float(np.float32(c)) * A > sur)
    return np.array([len(rows), (A < 0).sum(), dual.sum(), np.where(dual, float(np.float32(c)) * A, sur).sum(), sur.sum()], np.float64)


class Case:
    pass


_BUILT = {}


def planned(shape, M, positive=False):
    """The problem of (shape, M), built once per process and not to be modified: ppo_shape_cases.build's parameters and samples, the planned advantages and the
    cached log pi_old that realises the planned ratios.  positive: every advantage positive (same magnitudes and ratios): no row can be dual-clipped."""
    key = (shape, M, positive)
    if key in _BUILT:
        return _BUILT[key]
    din, A, hidden, seed, perturb, wide = SHAPES[shape]
    c = pc.build(din, A, hidden, M, seed, perturb, reference=False)
    q = Case()
    q.shape, q.M, q.din, q.A, q.hidden, q.wide = shape, M, din, A, tuple(hidden), wide
    q.theta, q.theta_old, q.s, q.a, q.R, q.low, q.high = c.theta, c.theta_old, c.s, c.a, c.R, c.low, c.high
    rng = np.random.RandomState(4100 + M)
    i = np.arange(M)
    q.target = np.array([PLAN[k % len(PLAN)][0] for k in i], np.float64)
    sign = np.array([1.0 if positive else PLAN[k % len(PLAN)][1] for k in i], np.float64)
    q.adv = (sign * (0.25 + 0.75 * rng.uniform(size=M))).astype(np.float32)
    q.logp64 = forward(q.theta, q.s, q.a, q.low, q.high)["logp"]
    q.logp_old = (q.logp64 - np.log(q.target)).astype(np.float32)
    q.ratio = np.exp(q.logp64 - q.logp_old.astype(np.float64))                        # what the fp32 cache realises
    q.cls = class_of(q.ratio, q.adv)
    _BUILT[key] = q
    return q


def plan_conditions(q):
    """The three conditions on the reference alone -> dict(classes present, the smallest distance from a threshold as a share of it, the smallest |A|)."""
    gap = min(float(np.abs(q.ratio / th - 1.0).min()) for th in THRESHOLDS)
    return dict(present=sorted(set(int(k) for k in q.cls)), gap=gap, a_min=float(np.abs(q.adv.astype(np.float64)).min()))


def expected_classes(M):
    """Every class at every M that has room for six; at M = 5 the five the plan begins with (see the module's text)."""
    return [DUAL, NEG_FLOW, NEG_LOW, POS_LOW, POS_HIGH] if M < 6 else [DUAL, NEG_FLOW, NEG_LOW, POS_LOW, POS_IN, POS_HIGH]
