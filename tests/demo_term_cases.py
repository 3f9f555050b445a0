"""Problems and the float64 reference of the PPO step with a demonstration term (mi_ppo_train_step_demo; test infrastructure, used by
test_demo_term_cases_host.py and test_zzzzzzzzzzz_demo_term_gpu.py).  Nothing here calls ppo.py, rollout.py or mi355/ beyond the initialiser the other case
modules use.

  loss = L_ppo(PPO rows) + c_d L_demo(demonstration rows)
L_ppo is oracle.ppo_oracle.ppo_losses (1 / M_p), with `vclip` its value term replaced by value_scale mean(max((V - R)^2, (V_c - R)^2)), V_c = V clamped into V_old +-
eps_v, and with `kl` plus beta mean_m KL(pi_old || pi_theta)[m] as tests/kl_penalty_cases.py spells it (its kl_terms / kl_bound / old_means / logstd_shift are used as
they are).  L_demo is clone_loss of tests/behaviour_cloning_cases.py, policy only, 1 / M_d: "nll" mean_m sum_a (z^2 / 2 + logstd + log(2 pi) / 2), "mse"
mean_m sum_a (mean - a_E)^2.  reference() is torch autograd over that sum in `dtype`.

Shapes: "A2" 67 -> 500 / 300 with 2 actions and "A3" 5 -> 36 / 20 with 3 actions (those of kl_penalty_cases), "W" 131 -> 500 / 300 with 2 actions (the wide layer 1).
Row counts (M_p, M_d): (5, 3) the boundary inside one wave; (33, 7) inside the second head block; (32, 32) on a block edge; (200, 57) a total of 257, the flat-buffer
route with a PPO part that alone would take the in-tile Adam; (257, 5) the chunked weight gradient.

A PPO problem is kl_penalty_cases.build (ppo_shape_cases.build with the log-std shift that conditions the KL).  The old values of the clipped value loss put sample i
into class i mod 3: inside the range (V_old = V + 0.05), V above it (V_old = V - 0.6) or below it (V_old = V + 0.6), eps_v = 0.2.  Demonstration states are drawn like
the PPO states; the expert's actions are the current policy's float64 means plus 0.3 N(0, 1), clamped into the action bounds.

conditioned(): the rules the other case modules use, on float64 values alone and with no sample exempted -- no ratio within GAP of a clip threshold, no value within
V_MARGIN of its clip edge and, outside the range, no return within V_MARGIN of the point (V + V_c) / 2 where the two value terms tie, and no layer pre-activation of
any of the M_p + M_d rows within KINK_TAU x the layer's largest |z| of zero."""
from collections import OrderedDict

import numpy as np
import torch

import behaviour_cloning_cases as bc
import kl_penalty_cases as kp
import ppo_shape_cases as pc
from oracle import ppo_oracle as po

SHAPES = OrderedDict([("A2", (67, 2, (500, 300), 2, 0.02)), ("A3", (5, 3, (36, 20), 11, 0.0231)), ("W", (131, 2, (500, 300), 5, 0.02))])
COUNTS = ((5, 3), (33, 7), (32, 32), (200, 57), (257, 5))
VARIANTS = OrderedDict([("plain", (False, False)), ("vclip", (True, False)), ("kl", (False, True)), ("kl_vclip", (True, True))])      # name -> (vclip, kl)
KINDS = bc.KINDS
C_D = 0.37
C_D32 = float(np.float32(C_D))                            # the coefficient as the kernels see it
BETA, BETA32 = kp.BETA, kp.BETA32
EPS_V = 0.2
EPS_V32 = float(np.float32(EPS_V))
GAP, V_MARGIN, KINK_TAU = 1e-4, 1e-3, pc.KINK_TAU
LOSS_REL, GRAD_REL, ADAM_ABS, ADAM_GMIN = bc.LOSS_REL, bc.GRAD_REL, bc.ADAM_ABS, bc.ADAM_GMIN
X3_GRAD_FLOOR, X3_GRAD_FACTOR = 1e-3, 4.0                # tests/test_j_ppo_bf16x3_gpu.py
NAMES = bc.NAMES
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def _t(x, dtype):
    return torch.from_numpy(np.asarray(x, np.float32)).to(dtype)


def build(shape, Mp, Md, seed_offset=0):
    din, A, hidden, seed, perturb = SHAPES[shape]
    c = pc.build(din, A, hidden, Mp, seed + seed_offset, perturb, reference=False)
    c.theta["policy/action_logstd"] = (c.theta_old["policy/action_logstd"] + kp.logstd_shift(A)).astype(np.float32)
    c.shape, c.Mp, c.Md = shape, Mp, Md
    rng = np.random.RandomState(7000 + 100 * Mp + Md + seed_offset)
    cand = (0.5 * rng.standard_normal((4 * Md + 8, din))).astype(np.float32)
    keep = np.flatnonzero(~pc.near_relu_kink(c.theta, np.concatenate([c.s, cand]))[Mp:])[:Md]
    assert len(keep) == Md, (len(keep), Md)
    c.ds = cand[keep]
    with torch.no_grad():
        th = {k: pc.t64(v) for k, v in c.theta.items()}
        mean_d, _, _ = po.policy_forward(th, pc.t64(c.ds), c.low, c.high)
        _, _, V = po.policy_forward(th, pc.t64(c.s), c.low, c.high)
    a_e = np.clip(mean_d.numpy() + 0.3 * rng.standard_normal((Md, A)), c.low, c.high).astype(np.float32)
    c.da = np.minimum(np.maximum(a_e, c.low), c.high)
    V = V.numpy()
    k = np.arange(Mp) % 3
    c.v_old = np.select([k == 0, k == 1], [V + 0.05, V - (EPS_V + 0.4)], V + (EPS_V + 0.4)).astype(np.float32)
    c.V64 = V
    return c


def demo_terms(mean, a_e, ls, kind):
    """torch: per-sample l[m] of the demonstration rows."""
    if kind == "mse":
        return ((mean - a_e) ** 2).sum(-1)
    z = (a_e - mean) / torch.exp(ls)
    return (0.5 * z * z + ls + HALF_LOG_2PI).sum(-1)


def reference(c, c_d, kind, vclip=False, kl=False, dtype=torch.float64, demo=True):
    """-> dict(scal: policy_loss, value_loss, entropy_loss, ratio_mean, ppo_loss (L_ppo), demo_loss, weighted, mean_sq_error, abs_terms, loss and with kl: kl,
    penalty, bound; grads: 13 arrays; mean [M_p, A] (the PPO rows' action means); ratio, value).  demo = False: L_ppo alone (the PPO reference)."""
    p = OrderedDict((k, _t(v, dtype).requires_grad_(True)) for k, v in c.theta.items())
    s, a, R, adv = (_t(x, dtype) for x in (c.s, c.a, c.R, c.adv))
    L = po.ppo_losses(p, {k: _t(v, dtype) for k, v in pc.old_names(c.theta_old).items()}, s, a, R, adv, c.low, c.high, pc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE)
    value_loss = L["value_loss"]
    if vclip:
        vo = _t(c.v_old, dtype)
        eps = torch.tensor(EPS_V32, dtype=dtype)
        vc = torch.minimum(torch.maximum(L["value"], vo - eps), vo + eps)
        value_loss = torch.maximum((L["value"] - R) ** 2, (vc - R) ** 2).mean() * pc.VALUE_SCALE
    loss = -L["policy_loss"] + value_loss - L["entropy_loss"]
    scal = {"policy_loss": float(L["policy_loss"].detach()), "value_loss": float(value_loss.detach()), "entropy_loss": float(L["entropy_loss"].detach()),
            "ratio_mean": float(L["ratio"].detach().mean())}
    ls = p["policy/action_logstd"]
    if kl:
        mean_o = torch.from_numpy(kp.old_means(c, dtype))
        lso = _t(c.theta_old["policy/action_logstd"], dtype)
        d, D = ls - lso, L["mean"] - mean_o
        klv = (d + 0.5 * torch.expm1(-2.0 * d) + D * D / (2.0 * torch.exp(2.0 * ls))).sum(-1).mean()
        pen = torch.tensor(BETA32, dtype=dtype) * klv
        loss = loss + pen
        klm, _, mag = kp.kl_terms(L["mean"].detach().numpy(), mean_o.numpy(), ls.detach().numpy(), lso.numpy())
        scal["kl"], scal["penalty"], scal["bound"] = float(klv.detach()), float(pen.detach()), kp.kl_bound(float(klm.mean()), float(mag.mean()))
    scal["ppo_loss"] = float(loss.detach())
    if demo:
        mean_d, _, _ = po.policy_forward(p, _t(c.ds, dtype), c.low, c.high)
        a_e = _t(c.da, dtype)
        dl = demo_terms(mean_d, a_e, ls, kind).mean()
        loss = loss + torch.tensor(float(np.float32(c_d)), dtype=dtype) * dl
        scal["demo_loss"], scal["weighted"] = float(dl.detach()), float(np.float32(c_d)) * float(dl.detach())
        scal["mean_sq_error"] = float(((mean_d - a_e) ** 2).sum(-1).mean().detach())
        z = ((a_e - mean_d) / torch.exp(ls)).detach().numpy()
        scal["abs_terms"] = float((z * z / 2 + np.abs(ls.detach().numpy()) + HALF_LOG_2PI).sum(1).mean()) if kind == "nll" else scal["demo_loss"]
    loss.backward()
    scal["loss"] = float(loss.detach())
    grads = OrderedDict((k, (v.grad if v.grad is not None else torch.zeros_like(v)).numpy()) for k, v in p.items())
    return dict(scal=scal, grads=grads, mean=L["mean"].detach().numpy(), ratio=L["ratio"].detach().numpy().reshape(-1), value=L["value"].detach().numpy())


def conditioned(c):
    """-> {rule: bool} on float64 values alone; every sample of both sides counts."""
    ref = reference(c, C_D, "nll", demo=False)
    r = ref["ratio"]
    gap = float(np.minimum(np.abs(r - (1 - pc.EPS)), np.abs(r - (1 + pc.EPS))).min())
    V, vo, R = ref["value"], c.v_old.astype(np.float64), c.R.astype(np.float64)
    edge = float(np.abs(np.abs(V - vo) - EPS_V32).min())
    vc = np.minimum(np.maximum(V, vo - EPS_V32), vo + EPS_V32)
    out = np.abs(V - vo) > EPS_V32
    tie = float(np.abs(R - 0.5 * (V + vc))[out].min()) if out.any() else np.inf
    kink = pc.near_relu_kink(c.theta, np.concatenate([c.s, c.ds]), KINK_TAU)
    return {"ratio_gap": gap >= GAP, "value_edge": edge >= V_MARGIN, "value_tie": tie >= V_MARGIN, "no_kink": not bool(kink.any()),
            "classes": bool(out.any()) and not bool(out.all()) if c.Mp >= 3 else True}


_BUILT = {}


def case(shape, Mp, Md):
    """The problem of (shape, M_p, M_d), built once per process and not to be modified: the first seed offset whose problem is well conditioned."""
    key = (shape, Mp, Md)
    if key not in _BUILT:
        for off in range(8):
            c = build(shape, Mp, Md, off)
            if all(conditioned(c).values()):
                c.seed_offset = off
                _BUILT[key] = c
                break
        else:
            raise AssertionError("no well-conditioned problem for %r" % (key,))
    return _BUILT[key]


_REFS = {}


def ref_of(shape, Mp, Md, variant, kind, dtype=torch.float64):
    """reference() of the case at C_D, computed once per process."""
    key = (shape, Mp, Md, variant, kind, dtype)
    if key not in _REFS:
        vclip, kl = VARIANTS[variant]
        _REFS[key] = reference(case(shape, Mp, Md), C_D, kind, vclip, kl, dtype)
    return _REFS[key]


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def demonstration_rows(rng, state, n, batch_size, steps):
    """The draw rule of RolloutBuffer.set_demonstrations, restated: state = [perm or None, cursor]; every step takes the next m = min(batch_size, n) rows of a
    permutation of the n rows; when fewer than m remain (or there is none yet) a fresh rng.permutation(n) is drawn first."""
    m, out = min(batch_size, n), []
    for _ in range(steps):
        if state[0] is None or n - state[1] < m:
            state[0], state[1] = rng.permutation(n), 0
        out.append(np.asarray(state[0][state[1]:state[1] + m], np.int32))
        state[1] += m
    return out
