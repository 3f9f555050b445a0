"""PPO problems at shapes other than the reference's (67 inputs, hidden 500 / 300, 2 actions), with their float64 reference (test infrastructure; used by
test_ppo_shape_cases_host.py, test_r_ppo_shapes_gpu.py, the op-level PPO tests of test_ops_gpu.py and the rollout-head test of test_l_rollout_batch_gpu.py).

build(input_dim, num_actions, hidden, M, seed, perturb) gives one problem:
  theta_old  mi355.init.init_ppo(seed, ...) with N(0, 0.05) biases and action_logstd = -0.5 + 0.07 a - 0.02 a^2 (every action its own, around -0.5);
  theta      theta_old + perturb x N(0, 1) on every variable;
  bounds     low[a] = -1 - 0.25 a, high[a] = 0.5 + 0.5 (a mod 3): no two actions alike, none [-1, 1];
  samples    0.5 x N(0, 1) states, the first M of 4 M draws that are not next to a ReLU kink of theta's trunks (near_relu_kink), the actions the OLD policy samples for them (clamped into the bounds), N(0, 1) returns and advantages;
  reference  oracle.ppo_oracle.ppo_losses on float64 tensors of those float32 values, all 13 gradients by autograd, log pi_old per sample.

The point of the perturbation is the zero-slope branch of min(r A, clip(r) A): conditions() measures, and the tests assert with conditions_met(), on the REFERENCE alone
  - 10 % .. 60 % of the samples on that branch (r > 1 + eps with A > 0, or r < 1 - eps with A < 0), at least one on each side;
  - no sample with min(|r - (1 - eps)|, |r - (1 + eps)|) < 1e-3: an fp32 kernel cannot then land on the other branch than float64 (an fp32 log-probability
    difference of size <= 3 is good to ~1e-6);
  - every ratio inside [1 / 20, 20].
The seed and the perturbation of every case are pinned in the tables below (found once by a search over seeds 1 .. 40 and a few perturbations scaled with
1 / sqrt(num_actions), since log r sums over the actions; the first hit was taken); nothing searches at test time.

The tolerances are the project's (tests/test_c_c3_ppo_gpu.py): 1e-4 relative (abs 1e-6) on the loss scalars, 2e-4 of each tensor's max on gradients, rtol 1e-4 /
atol 1e-5 on predicted actions and values."""
from collections import OrderedDict

import numpy as np
import torch

from oracle import ppo_oracle as po

EPS, VALUE_SCALE, ENTROPY_SCALE = 0.2, 1.0, 0.01
LOSS_KEYS = ("policy_loss", "value_loss", "entropy_loss", "loss", "ratio_mean")
LOSS_REL, LOSS_ABS, GRAD_REL = 1e-4, 1e-6, 2e-4
ACT_RTOL, ACT_ATOL = 1e-4, 1e-5
GAP_MIN, RATIO_MAX, SHARE_MIN, SHARE_MAX = 1e-3, 20.0, 0.10, 0.60
KINK_TAU = 1e-4

REF = (67, (500, 300))
# name -> (input_dim, num_actions, hidden, M, seed, perturb).  A: action counts on the reference trunk; B: trunk shapes the fused kernels take; C: shapes
# only the per-layer path takes (kin = 104 > 96; H2 = 324 > 320)
ENGINE_CASES = OrderedDict([
    ("A1-33", (67, 1, (500, 300), 33, 22, 0.03)), ("A1-77", (67, 1, (500, 300), 77, 5, 0.03)),
    ("A3-33", (67, 3, (500, 300), 33, 9, 0.0173)), ("A3-77", (67, 3, (500, 300), 77, 1, 0.0173)), ("A3-300", (67, 3, (500, 300), 300, 21, 0.0173)),
    ("A8-33", (67, 8, (500, 300), 33, 1, 0.0106)), ("A8-77", (67, 8, (500, 300), 77, 2, 0.0106)),
    ("B5-33", (5, 3, (36, 20), 33, 11, 0.0231)), ("B5-77", (5, 3, (36, 20), 77, 24, 0.0289)),
    ("B96-33", (96, 3, (132, 320), 33, 1, 0.0173)), ("B96-77", (96, 3, (132, 320), 77, 5, 0.0173)),
    ("B40-33", (40, 3, (100, 44), 33, 15, 0.0173)), ("B40-77", (40, 3, (100, 44), 77, 36, 0.0173)),
    ("C100-5", (100, 3, (64, 64), 5, 27, 0.0231)), ("C100-77", (100, 3, (64, 64), 77, 7, 0.0173)),
    ("C67-5", (67, 3, (64, 324), 5, 7, 0.0173)), ("C67-77", (67, 3, (64, 324), 77, 1, 0.0173)),
])
FUSED_CASES = [k for k in ENGINE_CASES if k[0] in "AB"]
PER_LAYER_CASES = [k for k in ENGINE_CASES if k[0] == "C"]

# op level (no trunk): (num_actions, M) -> (seed, spread): u = N(0, 1), u_old = u + spread x N(0, 1)
HEAD_ACTIONS, HEAD_SIZES = (1, 2, 3, 8), (1, 255, 256, 257, 300)
HEAD_CASES = OrderedDict([
    ((1, 1), (1, 0.2)), ((1, 255), (2, 0.3)), ((1, 256), (2, 0.3)), ((1, 257), (3, 0.3)), ((1, 300), (13, 0.3)),
    ((2, 1), (1, 0.1414)), ((2, 255), (3, 0.1414)), ((2, 256), (1, 0.1414)), ((2, 257), (7, 0.1414)), ((2, 300), (10, 0.1414)),
    ((3, 1), (2, 0.1155)), ((3, 255), (6, 0.1155)), ((3, 256), (5, 0.1155)), ((3, 257), (3, 0.0866)), ((3, 300), (5, 0.1155)),
    ((8, 1), (1, 0.0707)), ((8, 255), (1, 0.0707)), ((8, 256), (2, 0.0707)), ((8, 257), (2, 0.0707)), ((8, 300), (1, 0.0707)),
])


def bounds(A):
    a = np.arange(A)
    return (-1.0 - 0.25 * a).astype(np.float32), (0.5 + 0.5 * (a % 3)).astype(np.float32)


def logstd_of(A):
    a = np.arange(A, dtype=np.float64)
    return (-0.5 + 0.07 * a - 0.02 * a * a).astype(np.float32)


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float32).astype(np.float64))


def old_names(p):
    return OrderedDict((k.replace("policy/", "policy_old/", 1), v) for k, v in p.items())


def conditions(ratio, adv, eps=EPS):
    """The clipped-branch figures of a float64 ratio / advantage pair."""
    r, a = np.asarray(ratio, np.float64).reshape(-1), np.asarray(adv, np.float64).reshape(-1)
    hi, lo = (r > 1 + eps) & (a > 0), (r < 1 - eps) & (a < 0)
    return dict(share=float((hi | lo).mean()), n_hi=int(hi.sum()), n_lo=int(lo.sum()), n=len(r),
                gap=float(np.minimum(np.abs(r - (1 - eps)), np.abs(r - (1 + eps))).min()), ratio_min=float(r.min()), ratio_max=float(r.max()))


def conditions_met(c, single=False):
    """single: a one-sample problem cannot have a sample on each side nor a share between 10 % and 60 %: its one sample is on the sloped branch (a non-zero
    gradient to compare), at least 2 % away from ratio 1, and keeps the gap and range conditions."""
    if single:
        return (c["n"] == 1 and c["n_hi"] + c["n_lo"] == 0 and abs(c["ratio_min"] - 1) > 0.02 and c["gap"] >= GAP_MIN
                and 1 / RATIO_MAX <= c["ratio_min"] and c["ratio_max"] <= RATIO_MAX)
    return (SHARE_MIN <= c["share"] <= SHARE_MAX and c["n_hi"] >= 1 and c["n_lo"] >= 1 and c["gap"] >= GAP_MIN
            and 1 / RATIO_MAX <= c["ratio_min"] and c["ratio_max"] <= RATIO_MAX)


class Case:
    pass


def losses_and_grads(theta, theta_old, s, a, R, adv, low, high, dtype=torch.float64):
    """oracle.ppo_oracle.ppo_losses in `dtype` on float32 inputs -> (scalars, ratio, mean, value, the 13 gradients)."""
    t = lambda x: torch.from_numpy(np.asarray(x, np.float32)).to(dtype)      # noqa: E731
    p = OrderedDict((k, t(v).requires_grad_(True)) for k, v in theta.items())
    L = po.ppo_losses(p, {k: t(v) for k, v in old_names(theta_old).items()}, t(s), t(a), t(R), t(adv), low, high, EPS, VALUE_SCALE, ENTROPY_SCALE)
    L["loss"].backward()
    scal = {k: float(L[k].detach()) for k in LOSS_KEYS[:4]}
    scal["ratio_mean"] = float(L["ratio"].detach().mean())
    grads = OrderedDict((k, (v.grad if v.grad is not None else torch.zeros_like(v)).numpy()) for k, v in p.items())
    return scal, L["ratio"].detach().numpy().reshape(-1), L["mean"].detach().numpy(), L["value"].detach().numpy(), grads


def log_prob(theta, s, a, low, high, dtype=torch.float64):
    t = lambda x: torch.from_numpy(np.asarray(x, np.float32)).to(dtype)      # noqa: E731
    with torch.no_grad():
        mean, ls, _ = po.policy_forward({k: t(v) for k, v in theta.items()}, t(s), low, high)
        return po.normal_log_prob(t(a), mean, ls).sum(-1).numpy()


def near_relu_kink(theta, s, tau=KINK_TAU):
    """Samples with a ReLU pre-activation of theta's policy or value trunk within tau x that layer's max |z| of zero (float64).  Across such a kink a sample's
    whole contribution to a gradient column switches on or off: a discontinuity, not arithmetic (tests/test_j_ppo_bf16x3_gpu.py::near_kink, whose tau this is;
    the split-bf16 forward is good to ~1e-5 of a layer's max).  The ratio's own kinks are kept away by the gap condition."""
    th, x = {k: t64(v) for k, v in theta.items()}, t64(s)
    bad = torch.zeros(len(s), dtype=torch.bool)
    for k1, k2 in (("policy/dense", "policy/dense_1"), ("policy/dense_2", "policy/dense_3")):
        z1 = x @ th[k1 + "/kernel"] + th[k1 + "/bias"]
        z2 = torch.relu(z1) @ th[k2 + "/kernel"] + th[k2 + "/bias"]
        for z in (z1, z2):
            bad |= (z.abs() < tau * z.abs().max()).any(1)
    return bad.numpy()


def build(input_dim, A, hidden, M, seed, perturb, reference=True):
    from mi355.init import init_ppo
    c = Case()
    c.input_dim, c.A, c.hidden, c.M, c.seed, c.perturb = input_dim, A, tuple(hidden), M, seed, perturb
    c.low, c.high = bounds(A)
    rng = np.random.RandomState(1000 * seed + M)
    old = init_ppo(seed, input_dim, A, 1.0, hidden=hidden)
    for k in old:
        if k.endswith("bias"):
            old[k] = (0.05 * rng.standard_normal(old[k].shape)).astype(np.float32)
    old["policy/action_logstd"] = logstd_of(A)
    c.theta_old = old
    c.theta = OrderedDict((k, (v + perturb * rng.standard_normal(v.shape)).astype(np.float32)) for k, v in old.items())
    cand = (0.5 * rng.standard_normal((4 * M, input_dim))).astype(np.float32)
    keep = np.flatnonzero(~near_relu_kink(c.theta, cand))[:M]
    assert len(keep) == M, (len(keep), M)
    c.s = cand[keep]
    with torch.no_grad():
        mean_o, ls_o, v_o = po.policy_forward({k: t64(v) for k, v in old.items()}, t64(c.s), c.low, c.high)
    act = mean_o.numpy() + np.exp(ls_o.numpy()) * rng.standard_normal((M, A))
    c.a = np.clip(act, c.low, c.high).astype(np.float32)                     # clamped in float64 first, so the float32 values are inside the bounds
    c.a = np.minimum(np.maximum(c.a, c.low), c.high)
    c.R = (v_o.numpy() + rng.standard_normal(M)).astype(np.float32)
    c.adv = rng.standard_normal(M).astype(np.float32)
    if reference:
        c.scal, c.ratio, c.mean, c.value, c.grads = losses_and_grads(c.theta, c.theta_old, c.s, c.a, c.R, c.adv, c.low, c.high)
        c.logp_old = log_prob(c.theta_old, c.s, c.a, c.low, c.high)
        c.logp = log_prob(c.theta, c.s, c.a, c.low, c.high)
        c.cond = conditions(c.ratio, c.adv)
    return c


_BUILT = {}


def engine_case(name):
    """The problem of ENGINE_CASES[name], built once per process and not to be modified."""
    if name not in _BUILT:
        _BUILT[name] = build(*ENGINE_CASES[name])
    return _BUILT[name]


def predict_inputs(c, M):
    """States and noise of a predict call of M rows on case c's parameters (theta), with the float64 reference: greedy and sampled actions, values.  The noise is
    scaled past the bounds' width: rows 0, 3, 6, .. push every action with an even (row / 3 + index) above `high` and the others below `low`, rows 1, 4, .. the
    other way round, rows 2, 5, .. take N(0, 0.3) and stay mostly inside.  One row cannot clamp one action on both sides: with M >= 8 every action index is clamped at
    `low` in some row and at `high` in another (clamp_sides, asserted by the tests)."""
    rng = np.random.RandomState(7000 + 10 * M + c.A)
    s = (0.5 * rng.standard_normal((M, c.input_dim))).astype(np.float32)
    sigma = np.exp(c.theta["policy/action_logstd"].astype(np.float64))
    big = (3.0 + np.abs(rng.standard_normal((M, c.A)))) * (c.high - c.low) / sigma
    i, a = np.arange(M)[:, None], np.arange(c.A)[None, :]
    sign = np.where((i // 3 + a) % 2 == 0, 1.0, -1.0) * np.where(i % 3 == 0, 1.0, -1.0)
    noise = np.where(i % 3 == 2, 0.3 * rng.standard_normal((M, c.A)), sign * big).astype(np.float32)
    with torch.no_grad():
        mean, ls, value = po.policy_forward({k: t64(v) for k, v in c.theta.items()}, t64(s), c.low, c.high)
    raw = mean.numpy() + np.exp(ls.numpy()) * noise.astype(np.float64)
    sampled = np.clip(raw, c.low.astype(np.float64), c.high.astype(np.float64))
    sides = dict(low=(raw < c.low).any(0), high=(raw > c.high).any(0), inside=((raw > c.low) & (raw < c.high)).any())
    return dict(s=s, noise=noise, mean=mean.numpy(), sampled=sampled, value=value.numpy(), sides=sides)


# ---- op level: the head / loss kernel without the trunk ----
def head_case(A, M):
    """u, u_old, vraw drawn directly -> inputs and the float64 reference of mi_ppo_loss_fwd_bwd (clip 0.2, value scale 0.7, entropy scale 0.02) and of
    mi_policy_head.  Pinned (seed, spread) per (A, M) in HEAD_CASES."""
    seed, spread = HEAD_CASES[(A, M)]
    return build_head(A, M, seed, spread)


def head_reference(c, dtype=torch.float64):
    """The formulas of mi_ppo_loss_fwd_bwd in `dtype` (oracle.ppo_oracle's log-probability; clip 0.2, value scale 0.7, entropy scale 0.02) ->
    dict(losses [policy, value, entropy, total], ratio [M], du, dv, dls, mean)."""
    t = lambda x: torch.from_numpy(np.asarray(x, np.float32)).to(dtype)      # noqa: E731
    lo, hi = t(c.low), t(c.high)
    ut, lst, vt = t(c.u).requires_grad_(True), t(c.ls).requires_grad_(True), t(c.v).requires_grad_(True)
    mean = lo + ((torch.tanh(ut) + 1) / 2) * (hi - lo)
    mean_o = lo + ((torch.tanh(t(c.uo)) + 1) / 2) * (hi - lo)
    a = t(c.act)
    logp = po.normal_log_prob(a, mean, lst).sum(-1, keepdim=True)
    logpo = po.normal_log_prob(a, mean_o, t(c.lso)).sum(-1, keepdim=True)
    ratio = torch.exp(logp - logpo)
    adv = t(c.adv).unsqueeze(-1)
    pl = torch.minimum(ratio * adv, torch.clamp(ratio, 1 - EPS, 1 + EPS) * adv).mean()
    vl = ((vt - t(c.R)) ** 2).mean() * 0.7
    el = (0.5 + po.HALF_LOG_2PI + torch.log(torch.exp(lst))).sum() * 0.02
    loss = -pl + vl - el
    loss.backward()
    return dict(losses=[float(x.detach()) for x in (pl, vl, el, loss)], ratio=ratio.detach().numpy().reshape(-1), du=ut.grad.numpy(), dv=vt.grad.numpy(),
                dls=lst.grad.numpy(), mean=mean.detach().numpy())


def build_head(A, M, seed, spread):
    c = Case()
    rng = np.random.RandomState(100 * seed + 7)
    c.A, c.M = A, M
    c.low, c.high = bounds(A)
    c.u = rng.randn(M, A).astype(np.float32)
    c.uo = (c.u + spread * rng.randn(M, A)).astype(np.float32)
    c.ls = logstd_of(A)
    c.lso = (c.ls + 0.05 * (1 + np.arange(A) % 2)).astype(np.float32)
    c.v, c.R, c.adv = rng.randn(M).astype(np.float32), rng.randn(M).astype(np.float32), rng.randn(M).astype(np.float32)
    lo, hi = c.low.astype(np.float64), c.high.astype(np.float64)
    mean_o = lo + ((np.tanh(c.uo.astype(np.float64)) + 1) / 2) * (hi - lo)
    act = mean_o + np.exp(c.lso.astype(np.float64)) * rng.randn(M, A)         # the old policy's own samples, clamped into the bounds
    c.act = np.minimum(np.maximum(np.clip(act, c.low, c.high).astype(np.float32), c.low), c.high)
    ref = head_reference(c)
    c.losses, c.ratio, c.du, c.dv, c.dls, c.mean = ref["losses"], ref["ratio"], ref["du"], ref["dv"], ref["dls"], ref["mean"]
    c.ratio_mean = float(c.ratio.mean())
    c.cond = conditions(c.ratio, c.adv)
    # mi_policy_head: noise past the bounds on both sides for every action index (M >= 4), as in predict_inputs
    i, k = np.arange(M)[:, None], np.arange(A)[None, :]
    big = (3.0 + np.abs(rng.randn(M, A))) * (c.high - c.low) / np.exp(c.ls.astype(np.float64))
    sign = np.where((i // 3 + k) % 2 == 0, 1.0, -1.0) * np.where(i % 3 == 0, 1.0, -1.0)
    c.noise = np.where(i % 3 == 2, 0.3 * rng.randn(M, A), sign * big).astype(np.float32)
    raw = c.mean + np.exp(c.ls.astype(np.float64)) * c.noise.astype(np.float64)
    c.sampled = np.clip(raw, lo, hi)
    c.sides = dict(low=(raw < lo).any(0), high=(raw > hi).any(0), inside=bool(((raw > lo) & (raw < hi)).any()))
    return c
