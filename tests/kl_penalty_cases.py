"""Problems and the float64 reference of the adaptive KL penalty (test infrastructure; used by test_y_kl_penalty_gpu.py and test_kl_penalty_host.py).

Shapes and sizes are those of tests/test_s_value_clip_gpu.py: "A2" is 67 -> 500 / 300 with 2 actions (the <2> instantiation of the head / loss kernel), "A3" is
5 -> 36 / 20 with 3 actions (the <8> instantiation); M = 5 (one partial loss block), 33 (a second block that holds one sample) and 257 (the chunked
weight-gradient route).  A problem is ppo_shape_cases.build(.., reference=False) with theta's action_logstd replaced by logstd_old + (0.3, -0.25, 0.3, ..), so that
the log-std part of the KL is well conditioned (d = 0.3 gives 0.3 + expm1(-0.6) / 2 = 0.074 per action; at the 0.02 perturbation of build() it would be 1e-4 and
cancel to nothing in fp32).

reference(): oracle.ppo_oracle.policy_forward / ppo_losses in `dtype` with beta x mean KL added and autograd, the KL spelled as include/mi355_carla.h defines it:
  KL[m,a] = d + expm1(-2 d) / 2 + D^2 / (2 sigma^2) ,  d = ls - lso ,  D = mu - mu_o ,  sigma = exp(ls) ;  direction KL(pi_old || pi_theta).
mean_old: None (mu_o from the old policy's float64 forward) or the fp32 table a kernel reads (the cache form is checked against the very values it was given).

Bound on the KL scalar (kl_bound): 1e-4 KL + 2^-20 mean_m sum_a (|d| + 1/2 + e^{-2d} / 2 + D^2 / (2 sigma^2)) -- the project's relative tolerance on a loss scalar
plus fp32 rounding of the summands (2^-20: 16 ulp of 2^-24 on each, the style of the kl_row bound of test_w_vae_elementwise_gpu.py: the terms are formed from fp32
means with ~1e-6 of their own error, and the sum of the three cancels to a fifth of its largest term).  reference() asserts, on the float64 values alone, that the
mean KL is >= 0.1 and that the absolute floor is <= 1e-4 of it, so the bound is never dominated by the floor and no sample has to be left out."""
from collections import OrderedDict

import numpy as np
import torch

import ppo_shape_cases as pc
from oracle import ppo_oracle as po

SHAPES = OrderedDict([("A2", (67, 2, (500, 300), 2, 0.02)), ("A3", (5, 3, (36, 20), 11, 0.0231))])
MS = (5, 33, 257)
BETA = 0.7
BETA32 = float(np.float32(BETA))                          # the coefficient as the kernels see it
KL_REL, KL_FLOOR_ULP = 1e-4, 2.0 ** -20
KL_MIN, FLOOR_SHARE_MAX = 0.1, 1e-4
POLICY_NET = ("policy/dense/kernel", "policy/dense/bias", "policy/dense_1/kernel", "policy/dense_1/bias", "policy/action_mean/kernel", "policy/action_mean/bias",
              "policy/action_logstd")
VALUE_NET = ("policy/dense_2/kernel", "policy/dense_2/bias", "policy/dense_3/kernel", "policy/dense_3/bias", "policy/value/kernel", "policy/value/bias")


def logstd_shift(A):
    return np.where(np.arange(A) % 2 == 0, 0.3, -0.25).astype(np.float32)


def build(shape, M):
    din, A, hidden, seed, perturb = SHAPES[shape]
    c = pc.build(din, A, hidden, M, seed, perturb, reference=False)
    c.theta["policy/action_logstd"] = (c.theta_old["policy/action_logstd"] + logstd_shift(A)).astype(np.float32)
    return c


def kl_terms(mean, mean_o, ls, lso):
    """float64 numpy: KL[m] per sample, the mean part per sample, and the magnitude sum of the bound's floor per sample."""
    mean, mean_o, ls, lso = (np.asarray(x, np.float64) for x in (mean, mean_o, ls, lso))
    d, D = ls - lso, mean - mean_o
    q = D * D / (2.0 * np.exp(2.0 * ls))
    kl = (d + 0.5 * np.expm1(-2.0 * d) + q).sum(-1)
    mag = (np.abs(d) + 0.5 + 0.5 * np.exp(-2.0 * d) + q).sum(-1)
    return kl, q.sum(-1), mag


def kl_bound(kl_mean, mag_mean):
    return KL_REL * kl_mean + KL_FLOOR_ULP * mag_mean


def old_means(c, dtype=torch.float64):
    t = lambda x: torch.from_numpy(np.asarray(x, np.float32)).to(dtype)      # noqa: E731
    with torch.no_grad():
        mean_o, _, _ = po.policy_forward({k: t(v) for k, v in c.theta_old.items()}, t(c.s), c.low, c.high)
    return mean_o.numpy()


def reference(c, beta, dtype=torch.float64, mean_old=None, theta=None):
    """-> dict(scal: the five loss scalars + kl, penalty, loss (with the penalty), floor; grads: 13 arrays; mean, value; kl_m, mean_part_m per sample)."""
    t = lambda x: torch.from_numpy(np.asarray(x, np.float32)).to(dtype)      # noqa: E731
    theta = c.theta if theta is None else theta
    p = OrderedDict((k, t(v).requires_grad_(True)) for k, v in theta.items())
    L = po.ppo_losses(p, {k: t(v) for k, v in pc.old_names(c.theta_old).items()}, t(c.s), t(c.a), t(c.R), t(c.adv), c.low, c.high, pc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE)
    mean_o = torch.from_numpy(old_means(c, dtype)) if mean_old is None else t(mean_old)
    ls, lso = p["policy/action_logstd"], t(c.theta_old["policy/action_logstd"])
    d, D = ls - lso, L["mean"] - mean_o
    kl_m = (d + 0.5 * torch.expm1(-2.0 * d) + D * D / (2.0 * torch.exp(2.0 * ls))).sum(-1)
    kl = kl_m.mean()
    beta_t = torch.tensor(float(np.float32(beta)), dtype=dtype)
    loss = L["loss"] + beta_t * kl
    loss.backward()
    scal = {k: float(L[k].detach()) for k in pc.LOSS_KEYS[:3]}
    scal["ratio_mean"] = float(L["ratio"].detach().mean())
    scal["kl"], scal["penalty"], scal["loss"] = float(kl.detach()), float((beta_t * kl).detach()), float(loss.detach())
    grads = OrderedDict((k, (v.grad if v.grad is not None else torch.zeros_like(v)).numpy()) for k, v in p.items())
    klm, part, mag = kl_terms(L["mean"].detach().numpy(), mean_o.numpy(), ls.detach().numpy(), lso.numpy())
    scal["floor"] = KL_FLOOR_ULP * float(mag.mean())
    scal["bound"] = kl_bound(float(klm.mean()), float(mag.mean()))
    return dict(scal=scal, grads=grads, mean=L["mean"].detach().numpy(), value=L["value"].detach().numpy(), kl_m=klm, mean_part_m=part)


def well_conditioned(ref):
    """The conditions every problem is asserted to meet, on float64 values alone."""
    return ref["scal"]["kl"] >= KL_MIN and ref["scal"]["floor"] <= FLOOR_SHARE_MAX * ref["scal"]["kl"] and bool(np.all(ref["kl_m"] >= 0.0))


_BUILT = {}


def case(shape, M):
    """(problem, float64 reference at BETA with the old policy's float64 means), built once per process and not to be modified."""
    if (shape, M) not in _BUILT:
        c = build(shape, M)
        ref = reference(c, BETA)
        assert well_conditioned(ref), (shape, M, ref["scal"])
        _BUILT[(shape, M)] = (c, ref)
    return _BUILT[(shape, M)]


def adapted(coef, target, kl):
    """The paper's rule, spelled independently of ppo.adapted_kl_coef."""
    if target is None:
        return coef
    if kl < target / 1.5:
        return coef / 2.0
    if kl > target * 1.5:
        return coef * 2.0
    return coef
