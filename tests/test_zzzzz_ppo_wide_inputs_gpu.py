"""The fused PPO kernels at more than 96 inputs (mi_ppo_set_wide_inputs, csrc/ppo_fused.hip ppo_l1_wide_kernel) against the float64 oracle and against themselves.
Problems and references: tests/ppo_wide_cases.py (conditions on the reference: tests/test_ppo_wide_host.py).  Bounds are those of tests/test_r_ppo_shapes_gpu.py: fp32
1e-4 relative (abs 1e-6) on loss scalars, 2e-4 of each tensor's max on gradients, rtol 1e-4 / atol 1e-5 on actions and values; bf16x3 1e-4 on loss scalars and
max(1e-3, 4 x the fp32 oracle's own distance from float64) on gradients.  Every test prints the worst figure it saw next to its bound.

  1  gradients, losses, predict against float64: mode 1 fp32, mode 2 fp32, mode 1 bf16x3; contiguous tensors and rows of a table whose unnamed rows are NaN
  2  the one-call steps: TF-Adam on the reference's gradients, the gather, the cache, repeatability, the zero padding rows, the gathered copy
  3  what the per-layer path refuses runs in mode 1 -- and is still refused in mode 0 (these fail on a tree without the setting)
  4  nothing moves at 96 inputs and below, nor past 1024; tables of 2 GiB are refused before any launch
  5  the rollout step and both rollout buffers on a 103-input policy

Tables: in mode 1 the named rows are scattered over M + 7 rows.  In mode 2 layer 1 is ppo_l1_kernel, whose documented precondition (include/mi355_carla.h) is that the
first entries of the table row BEHIND a gathered row are finite -- it multiplies them by zero weights --, so there the named rows are the table's last M rows in
shuffled order and the NaN rows come first: every unnamed row is still NaN, and every row behind a named one is a named one or the end of the table."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ppo_shape_cases as pc  # noqa: E402
import ppo_wide_cases as wc  # noqa: E402
from oracle import vae_oracle as vo  # noqa: E402
from mi355 import lib as milib  # noqa: E402
from ppo import _adam_alpha  # noqa: E402
from rollout_gpu_common import bitwise, flat_state, make_pair  # noqa: E402

LR = 1e-4
ALPHA = _adam_alpha(LR, 0.9, 0.999)
X3_LOSS_REL, X3_GRAD_FLOOR, X3_GRAD_FACTOR = 1e-4, 1e-3, 4.0
MODES = [(1, "fp32"), (2, "fp32"), (1, "bf16x3")]
INF = float("inf")


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


class Rig:
    """One engine per shape; a test loads a case (its parameters and samples) and picks the mode and the precision."""

    def __init__(self, shape):
        from mi355.ppo_device import PpoDevice
        din, A, hidden = shape
        low, high = pc.bounds(A)
        assert hasattr(PpoDevice, "set_wide_inputs"), "this tree has no wide-input setting"
        self.d = PpoDevice(din, A, low, high, pc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE, hidden=hidden, max_batch=320)
        self.c = None

    def load(self, c, mode, precision="fp32"):
        d = self.d
        if d.precision != "fp32":
            d.set_precision("fp32")
        d.set_wide_inputs(mode)
        if precision != "fp32":
            d.set_precision(precision)
        d.set_max_grad_norm(None)
        assert d.engine_wide_inputs() == mode and d.precision == precision
        if c is not self.c:
            up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(d.device)      # noqa: E731
            self.c, self.s, self.a, self.R, self.adv = c, up(c.s), up(c.a), up(c.R), up(c.adv)
        self.reset()
        return self

    def reset(self):
        d = self.d
        d.load_params(self.c.theta, pc.old_names(self.c.theta_old))
        d.adam_m.zero_(); d.adam_v.zero_(); d.grads.zero_()

    def used(self):
        used = torch.zeros(self.d.n_flat, dtype=torch.bool, device=self.d.device)
        for _, (o_, s_) in self.d.layout.items():
            used[o_:o_ + s_] = True
        return used

    def state(self):
        d = self.d
        return [d.params.clone(), d.adam_m.clone(), d.adam_v.clone(), d.losses.clone()]

    def table(self, mode, seed=0):
        """The samples as rows of tables (see the module docstring) -> dict(s, a, R, adv, v_old, rows, pos); every unnamed row of every table is NaN."""
        c, d = self.c, self.d
        M = c.M
        T = M + 7
        rng = np.random.RandomState(M + c.A + seed)
        pos = (rng.permutation(T)[:M] if mode == 1 else 7 + rng.permutation(M)).astype(np.int32)

        def tab(x):
            t = np.full((T,) + x.shape[1:], np.nan, np.float32)
            t[pos] = x
            return torch.from_numpy(t).to(d.device)
        return dict(s=tab(c.s), a=tab(c.a), R=tab(c.R), adv=tab(c.adv), v_old=tab(np.zeros(M, np.float32)), rows=torch.from_numpy(pos).to(d.device), pos=pos, T=T)


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(name, mode, precision="fp32"):
        shape = wc.WIDE_CASES[name][:3]
        if shape not in made:
            made[shape] = Rig(shape)
        return made[shape].load(wc.wide_case(name), mode, precision)
    yield get
    for r in made.values():
        r.d.close()


_G32 = {}


def grad_bounds(name, precision, c):
    if precision == "fp32":
        return {k: pc.GRAD_REL for k in c.grads}
    if name not in _G32:
        g32 = pc.losses_and_grads(c.theta, c.theta_old, c.s, c.a, c.R, c.adv, c.low, c.high, dtype=torch.float32)[4]
        _G32[name] = {k: rel_err(g32[k], c.grads[k]) for k in c.grads}
    return {k: max(X3_GRAD_FLOOR, X3_GRAD_FACTOR * _G32[name][k]) for k in c.grads}


def check_losses(L, c, rel, tag):
    worst = 0.0
    for got, key in zip(L[:5], pc.LOSS_KEYS):
        worst = max(worst, abs(float(got) - c.scal[key]) / max(abs(c.scal[key]), 1e-30))
        assert float(got) == pytest.approx(c.scal[key], rel=rel, abs=pc.LOSS_ABS), (tag, key, float(got), c.scal[key])
    return worst


def check_gradients(r, name, precision, tag):
    c, d = r.c, r.d
    L = d.losses.cpu().numpy().astype(np.float64)
    worst_l = check_losses(L, c, pc.LOSS_REL if precision == "fp32" else X3_LOSS_REL, tag)
    g = d.export_grads()
    bound = grad_bounds(name, precision, c)
    err = {k: rel_err(g[k], c.grads[k]) for k in c.grads}
    k_w = max(err, key=lambda k: err[k] / bound[k])
    print("\n%s: loss scalars %.2e (bound 1e-4), worst gradient %.2e of max (bound %.1e, %s)" % (tag, worst_l, err[k_w], bound[k_w], k_w))
    bad = {k: (err[k], bound[k]) for k in err if not err[k] <= bound[k]}
    assert not bad, (tag, bad)


# ---------------------------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("mode,precision", MODES, ids=lambda x: str(x))
@pytest.mark.parametrize("name", wc.FUSED_WIDE)
def test_gradient_pass_against_float64(rigs, name, mode, precision):
    """forward_backward on contiguous tensors, then the same pass on table rows (train_step_vclip with adam = 0 and eps_v = inf: the gather form that stops with the
    gradients in the buffer); both against float64, and the second bitwise the first -- a NaN of an unnamed row that reached layer 1 would show in both checks."""
    r = rigs(name, mode, precision)
    c, d = r.c, r.d
    assert d.fused_ok() and d.kin == wc.kin_of(c.input_dim) and d.engine_precision() == (milib.MI_F32 if precision == "fp32" else milib.MI_BF16X3)
    d.forward_backward(r.s, r.a, r.R, r.adv, c.M, 1.0 / c.M, 1.0)
    check_gradients(r, name, precision, "%s mode %d %s contiguous" % (name, mode, precision))
    first, l_first = d.grads.clone(), d.losses.clone()
    t = r.table(mode)
    d.grads.fill_(4.25)
    d.losses.fill_(-3.0)
    d.train_step_vclip(None, t["s"], t["a"], t["R"], t["adv"], None, t["v_old"], INF, t["rows"], c.M, 1.0 / c.M, 1.0, ALPHA, adam=False)
    check_gradients(r, name, precision, "%s mode %d %s table rows" % (name, mode, precision))
    used = r.used()
    assert torch.equal(d.grads[used].view(torch.int32), first[used].view(torch.int32))
    assert torch.equal(d.losses.view(torch.int32), l_first.view(torch.int32))


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("shape", [k for k in wc.SHAPES if k != "W1025"])
def test_predict_sampled_and_greedy(rigs, shape, mode):
    """M = 1, 9, 33: actions (noise past the bounds on both sides of every action index), values, the action_mean table; rows past M are nobody's."""
    name = next(k for k in wc.FUSED_WIDE if k.startswith(shape + "-"))
    r = rigs(name, mode)
    c, d = r.c, r.d
    worst_a = worst_v = 0.0
    for M in (1, 9, 33):
        p = pc.predict_inputs(c, M)
        sd, nz = torch.from_numpy(p["s"]).to(d.device), torch.from_numpy(p["noise"]).to(d.device)
        for greedy in (False, True):
            act = torch.full((M + 2, c.A), -777.0, device=d.device)
            val = torch.full((M + 2,), -777.0, device=d.device)
            d.action_mean.fill_(-777.0)
            d.predict(sd, M, None if greedy else nz, greedy, act, val)
            a, v, mean = act.cpu().numpy(), val.cpu().numpy(), d.action_mean.cpu().numpy()
            want = p["mean"] if greedy else p["sampled"]
            worst_a = max(worst_a, float(np.abs(a[:M] - want).max()))
            worst_v = max(worst_v, float(np.abs(v[:M] - p["value"]).max()))
            assert np.allclose(a[:M], want, rtol=pc.ACT_RTOL, atol=pc.ACT_ATOL), (M, greedy, float(np.abs(a[:M] - want).max()))
            assert np.allclose(v[:M], p["value"], rtol=pc.ACT_RTOL, atol=pc.ACT_ATOL), (M, greedy)
            assert np.allclose(mean[:M], p["mean"], rtol=pc.ACT_RTOL, atol=pc.ACT_ATOL), (M, greedy)
            assert np.all(a[M:] == -777.0) and np.all(v[M:] == -777.0) and np.all(mean[M:] == -777.0)
    print("\n%s mode %d: worst |action diff| %.2e, |value diff| %.2e (rtol 1e-4, atol 1e-5)" % (shape, mode, worst_a, worst_v))


# ---------------------------------------------------------------------------------------------------------------------------------------- 2
@pytest.fixture(scope="module")
def recording_comm():
    L = milib.get()
    hcomm, log = ctypes.c_void_p(), np.zeros((256, 4), np.int64)
    L.mi_comm_init_recording(ctypes.addressof(hcomm), 0, 1, log.ctypes.data, 256)
    yield hcomm
    L.mi_comm_destroy(hcomm)


def check_adam(r, tag):
    """Parameters after ONE step from the case's theta against oracle.vae_oracle.AdamTF on the float64 reference's gradients (tests/test_r_ppo_shapes_gpu.py)."""
    c, d = r.c, r.d
    want = {k: v.copy() for k, v in c.theta.items()}
    grads = {k: v.astype(np.float32) for k, v in c.grads.items()}
    vo.AdamTF({k: v.shape for k, v in want.items()}).step(want, grads, LR)
    got = d.export_params()
    worst = 0.0
    for k in want:
        sig = np.abs(grads[k]) > 1e-6                     # where Adam's first step is +-lr regardless of rounding
        assert sig.any(), k
        worst = max(worst, float(np.abs(got[k][sig] - want[k][sig]).max()))
        assert np.allclose(got[k][sig], want[k][sig], rtol=0, atol=2e-6), (tag, k, float(np.abs(got[k][sig] - want[k][sig]).max()))
        assert np.abs(got[k] - c.theta[k]).max() <= 1.01e-4 + 1e-9, (tag, k)
    worst_l = check_losses(d.losses.cpu().numpy().astype(np.float64), c, 1e-4, tag)
    print("\n%s: parameters after the step, worst |diff| %.2e (bound 2e-6); loss scalars %.2e (bound 1e-4)" % (tag, worst, worst_l))


def padding_rows(d, flat):
    """Rows din .. kin - 1 of both first-layer kernels of a flat buffer."""
    out = []
    for name in ("policy/dense/kernel", "policy/dense_2/kernel"):
        o, s = d.layout[name]
        out.append(flat[o:o + s].view(d.kin, -1)[d.input_dim:])
    return out


@pytest.mark.parametrize("name", wc.FUSED_WIDE)
def test_one_call_steps(rigs, recording_comm, name):
    """Mode 1, fp32.  train_step against TF-Adam on the reference's gradients; a second run bitwise the first; train_step_idx on scattered table rows (NaN elsewhere)
    bitwise train_step, and s_gath bitwise the gathered rows; the step from the cached log pi_old within 1e-7 of the step that evaluates the old policy; train_step_dp on
    a recording communicator against TF-Adam; after three steps the padding rows of W1 and of its Adam slots are exactly 0.0."""
    r = rigs(name, 1)
    c, d = r.c, r.d
    M = c.M
    args = (M, 1.0 / M, 1.0, ALPHA)
    d.train_step(r.s, r.a, r.R, r.adv, *args)
    check_adam(r, name + " train_step")
    one = r.state()
    assert not torch.equal(one[0], torch.from_numpy(d._to_flat(c.theta)).to(d.device))
    r.reset()
    d.train_step(r.s, r.a, r.R, r.adv, *args)
    assert bitwise(r.state(), one), "two runs differ"
    # the gather
    t = r.table(1)
    r.reset()
    d.workspace[:M * c.input_dim * 4].view(torch.float32).fill_(-777.0)               # s_gath: the engine's workspace begins with the padded-state buffer
    d.train_step_idx(t["s"], t["a"], t["R"], t["adv"], None, t["rows"], *args)
    assert bitwise(r.state(), one), float((d.params - one[0]).abs().max())
    gath = d.workspace[:M * c.input_dim * 4].view(torch.float32).view(M, c.input_dim)
    assert torch.equal(gath.view(torch.int32), r.s.view(torch.int32)), "s_gath is not the gathered minibatch"
    # the cache
    lp = torch.full((M + 3,), float("nan"), device=d.device)
    r.reset()
    d.logp_old(r.s, r.a, M, lp)
    got_lp = lp.cpu().numpy()
    assert np.isnan(got_lp[M:]).all()
    err = np.abs(got_lp[:M] - c.logp_old).max() / np.abs(c.logp_old).max()
    assert err <= 1e-4, err
    d.train_step(r.s, r.a, r.R, r.adv, *args, logp_old=lp)
    p_cache, p_one = d.export_params(), d._from_flat(one[0].cpu().numpy())
    diff = {k: float(np.abs(p_cache[k] - p_one[k]).max()) for k in p_one}
    k_w = max(diff, key=diff.get)
    print("%s: log pi_old %.2e of max (bound 1e-4); cached against in-step old policy, worst |parameter diff| %.3e (%s; bound 1e-7)" % (name, err, diff[k_w], k_w))
    assert all(v <= 1e-7 for v in diff.values()), diff
    # data parallel form on the recording communicator: the flat route
    L = milib.get()
    n0 = L.mi_comm_recorded(recording_comm)
    r.reset()
    d.train_step_dp(recording_comm, t["s"], t["a"], t["R"], t["adv"], None, t["rows"], *args)
    assert L.mi_comm_recorded(recording_comm) == n0 + 1
    check_adam(r, name + " train_step_dp")
    # two more steps: the zero padding rows
    for _ in range(2):
        d.train_step_idx(t["s"], t["a"], t["R"], t["adv"], None, t["rows"], *args)
    for flat in (d.params, d.params_old, d.adam_m, d.adam_v):
        for rows in padding_rows(d, flat):
            assert rows.shape[0] == d.kin - d.input_dim and bool((rows == 0.0).all()), name
    assert bool(torch.isfinite(d.params).all())


# ---------------------------------------------------------------------------------------------------------------------------------------- 3
REFUSED = ["W131-33", "W515-33", "W131-257", "W515-257"]


@pytest.mark.parametrize("name", REFUSED)
def test_what_was_refused_runs_in_mode_1(rigs, name):
    from mi355.ppo_device import N_KL_STATS, N_STATS
    r = rigs(name, 1)
    c, d = r.c, r.d
    M = c.M
    args = (M, 1.0 / M, 1.0, ALPHA)
    t = r.table(1)
    d.train_step(r.s, r.a, r.R, r.adv, *args)
    one = r.state()
    # value clipping with eps_v = inf is the plain step, bit for bit
    r.reset()
    d.train_step_vclip(None, t["s"], t["a"], t["R"], t["adv"], None, t["v_old"], INF, t["rows"], *args)
    assert bitwise(r.state(), one)
    # the KL penalty with beta = 0 adds nothing
    r.reset()
    d.train_step_kl(None, r.s, r.a, r.R, r.adv, None, None, 0.0, None, *args)
    assert all(torch.equal(x, y) for x, y in zip(r.state()[:3], one[:3]))
    assert torch.equal(d.losses[:5], one[3][:5]) and float(d.kl_losses[0]) > 0 and float(d.kl_losses[1]) == 0.0
    # the old-policy cache
    r.reset()
    lp, lp2 = torch.full((M,), float("nan"), device=d.device), torch.full((M,), float("nan"), device=d.device)
    mu = torch.full((M, c.A), float("nan"), device=d.device)
    d.logp_old(r.s, r.a, M, lp)
    d.old_policy_cache(r.s, r.a, M, lp2, mu)
    assert bitwise(lp, lp2) and bool(torch.isfinite(mu).all())
    # statistics at theta == theta_old: every KL sum is exactly 0
    d.params.copy_(d.params_old)
    T = t["T"]
    lp_t, mu_t = torch.full((T,), float("nan"), device=d.device), torch.full((T, c.A), float("nan"), device=d.device)
    lp_t[t["rows"].long()] = lp
    mu_t[t["rows"].long()] = mu
    stats = torch.full((N_STATS,), -777.0, dtype=torch.float64, device=d.device)
    scratch = torch.zeros(d.stats_scratch_doubles(M), dtype=torch.float64, device=d.device)
    d.update_stats(t["s"], t["a"], t["R"], lp_t, t["rows"], M, stats, scratch)
    st = stats.cpu().numpy()
    assert st[0] == M and st[1] == 0.0 and st[2] == 0.0 and st[3] == 0.0 and st[4] == M, st
    kst = torch.full((N_KL_STATS,), -777.0, dtype=torch.float64, device=d.device)
    ksc = torch.zeros(d.kl_stats_scratch_doubles(M), dtype=torch.float64, device=d.device)
    d.kl_stats(t["s"], mu_t, t["rows"], M, kst, ksc)
    assert kst.cpu().numpy().tolist() == [float(M), 0.0, 0.0, 0.0], kst
    # the split mode is accepted
    d.set_precision("bf16x3")
    assert d.engine_precision() == milib.MI_BF16X3 and d.fused_ok()
    d.set_precision("fp32")
    # clipping by the global norm: the gradient buffer x the factor, then mi_ppo_apply_adam, bit for bit
    r.reset()
    d.forward_backward(r.s, r.a, r.R, r.adv, M, 1.0 / M, 1.0)
    grad = d.grads.clone()
    d.grad_norm(INF)
    norm = float(d.grad_clip[0])
    clipped = 0
    for limit in (0.5, 0.5 * norm):                                                  # (the second limit clips whatever this problem's norm is)
        r.reset()
        d.set_max_grad_norm(limit)
        d.train_step(r.s, r.a, r.R, r.adv, *args)
        got, rec = r.state()[:3], d.grad_clip.clone()
        d.set_max_grad_norm(None)
        assert float(rec[0]) == pytest.approx(norm, rel=1e-6) and (float(rec[1]) < 1.0) == (norm > limit), (rec, norm, limit)
        clipped += float(rec[1]) < 1.0
        r.reset()
        d.grads.copy_(grad)
        d.grads.mul_(rec[1])
        d.apply_adam(ALPHA)
        assert bitwise(r.state()[:3], got), limit
    print("\n%s: gradient norm %.4f; clipped at %d of the limits 0.5 and norm / 2" % (name, norm, clipped))
    assert clipped >= 1


def test_the_mode_survives_ensure_batch():
    from mi355.ppo_device import PpoDevice
    c = wc.wide_case("W131-33")
    d = PpoDevice(c.input_dim, c.A, c.low, c.high, pc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE, hidden=c.hidden, max_batch=16, wide_inputs=1, precision="bf16x3")
    try:
        h = d.handle
        assert d.fused_ok() and d.engine_wide_inputs() == 1
        d.ensure_batch(64)
        assert d.handle != h and d.max_batch >= 64 and d.fused_ok() and d.engine_wide_inputs() == 1 and d.engine_precision() == milib.MI_BF16X3
        with pytest.raises(milib.MiError):                                           # back to the narrow range: the split mode would lose its kernels
            d.set_wide_inputs(0)
        assert d.engine_wide_inputs() == 1 and d.wide_inputs == 1
    finally:
        d.close()


@pytest.mark.parametrize("name", ["W131-33", "W515-33"])
def test_mode_0_refuses_what_it_refuses_today(rigs, name):
    """The same calls in mode 0: MI_ERR_SHAPE before anything is launched (output buffers and parameters keep their contents), and the split mode is not accepted."""
    from mi355.ppo_device import N_KL_STATS, N_STATS
    r = rigs(name, 0)
    c, d = r.c, r.d
    M = c.M
    assert not d.fused_ok() and d.engine_wide_inputs() == 0
    args = (M, 1.0 / M, 1.0, ALPHA)
    rows = torch.arange(M, dtype=torch.int32, device=d.device)
    lp = torch.full((M,), float("nan"), device=d.device)
    mu = torch.full((M, c.A), float("nan"), device=d.device)
    zeros = torch.zeros(M, device=d.device)
    stats = torch.full((N_STATS,), -777.0, dtype=torch.float64, device=d.device)
    kst = torch.full((N_KL_STATS,), -777.0, dtype=torch.float64, device=d.device)
    scratch = torch.zeros(d.stats_scratch_doubles(M), dtype=torch.float64, device=d.device)
    before = r.state()
    calls = {
        "mi_ppo_train_step_idx": lambda: d.train_step_idx(r.s, r.a, r.R, r.adv, None, rows, *args),
        "mi_ppo_train_step_vclip": lambda: d.train_step_vclip(None, r.s, r.a, r.R, r.adv, None, zeros, INF, None, *args),
        "mi_ppo_train_step_kl": lambda: d.train_step_kl(None, r.s, r.a, r.R, r.adv, None, None, 0.0, None, *args),
        "mi_ppo_old_policy_cache": lambda: d.old_policy_cache(r.s, r.a, M, lp, mu),
        "mi_ppo_logp_old": lambda: d.logp_old(r.s, r.a, M, lp),
        "mi_ppo_update_stats_idx": lambda: d.update_stats(r.s, r.a, r.R, zeros, rows, M, stats, scratch),
        "mi_ppo_kl_stats_idx": lambda: d.kl_stats(r.s, torch.zeros(M, c.A, device=d.device), rows, M, kst, scratch),
        "mi_ppo_set_precision": lambda: d.set_precision("bf16x3"),
    }
    for entry, call in calls.items():
        with pytest.raises(milib.MiError, match=entry + r" failed \(-2\)"):
            call()
    torch.cuda.synchronize()
    assert bitwise(r.state(), before) and bool(torch.isnan(lp).all()) and bool(torch.isnan(mu).all()) and bool((stats == -777.0).all()) and bool((kst == -777.0).all())
    assert d.engine_precision() == milib.MI_F32 and d.precision == "fp32"
    # ... and the plain step still runs, on the per-layer path, against the same reference
    d.train_step(r.s, r.a, r.R, r.adv, *args)
    check_adam(r, name + " mode 0 (per-layer)")


# ---------------------------------------------------------------------------------------------------------------------------------------- 4
_NARROW = {}


def narrow_case(key):
    if key not in _NARROW:
        _NARROW[key] = pc.engine_case("B96-33") if key == "B96" else pc.build(67, 2, (500, 300), 33, 3, 0.02, reference=False)
    return _NARROW[key]


@pytest.mark.parametrize("key", ["REF67", "B96"])
def test_narrow_shapes_run_the_same_launches_in_every_mode(key):
    """The reference shape (67 inputs) and B96 of ppo_shape_cases: two in-tile Adam steps, then a gradient pass into a buffer full of 4.25 -- parameters, Adam slots,
    losses and the gradient buffer of modes 1 and 2 are bitwise those of mode 0."""
    from mi355.ppo_device import PpoDevice
    c = narrow_case(key)
    d = PpoDevice(c.input_dim, c.A, c.low, c.high, pc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE, hidden=c.hidden, max_batch=64)
    try:
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(d.device)      # noqa: E731
        s, a, R, adv = up(c.s), up(c.a), up(c.R), up(c.adv)
        outs = []
        for mode in (0, 1, 2):
            d.set_wide_inputs(mode)
            assert d.fused_ok()
            d.load_params(c.theta, pc.old_names(c.theta_old))
            d.adam_m.zero_(); d.adam_v.zero_()
            for _ in range(2):
                d.train_step(s, a, R, adv, c.M, 1.0 / c.M, 1.0, ALPHA)
            st = [d.params.clone(), d.adam_m.clone(), d.adam_v.clone(), d.losses.clone()]
            d.grads.fill_(4.25)
            d.forward_backward(s, a, R, adv, c.M, 1.0 / c.M, 1.0)
            outs.append(st + [d.grads.clone(), d.losses.clone()])
        assert not torch.equal(outs[0][0], torch.from_numpy(d._to_flat(c.theta)).to(d.device))
        assert bitwise(outs[1], outs[0]) and bitwise(outs[2], outs[0])
    finally:
        d.close()


def past_the_limit(rigs):
    r = rigs("W1025-33", 0)
    c, d = r.c, r.d
    outs = []
    for mode in (0, 1, 2):
        r.load(c, mode)
        assert not d.fused_ok()
        d.train_step(r.s, r.a, r.R, r.adv, c.M, 1.0 / c.M, 1.0, ALPHA)
        outs.append(r.state())
        check_adam(r, "W1025-33 mode %d (per-layer)" % mode)
    return r, outs


def test_past_the_limit_every_mode_is_the_per_layer_path(rigs):
    """1025 inputs (kin = 1032): fused_ok() is False in every mode, the step runs on the per-layer path against the same reference, its loss scalars (the forward
    pass and the loss kernel) are bitwise those of mode 0, and what only the fused kernels do is refused."""
    r, outs = past_the_limit(rigs)
    c, d = r.c, r.d
    assert bitwise(outs[1][3], outs[0][3]) and bitwise(outs[2][3], outs[0][3])
    with pytest.raises(milib.MiError, match=r"mi_ppo_logp_old failed \(-2\).*inputs <= 1024"):
        d.logp_old(r.s, r.a, c.M, torch.zeros(c.M, device=d.device))
    with pytest.raises(milib.MiError, match=r"mi_ppo_set_precision failed \(-2\)"):
        d.set_precision("bf16x3")


def test_past_the_limit_mode_1_is_bitwise_mode_0(rigs):
    """Parameters, Adam slots and losses of W1025 in modes 1 and 2 are bitwise those of mode 0: every mode runs the per-layer path, and that path adds the row splits
    of its filter and bias gradients in a fixed order (mi_gemm_wgrad_ws / mi_colsum_ws on slabs in the engine's workspace).  It used to add them with fp32 atomics: three
    mode-0 runs of this very step then differed from each other by up to 3.7e-9 in Adam's first moment (profiles/r28_ppo_wide_inputs.md), so the comparison had no
    meaning.  A second mode-0 run is compared as well."""
    r, outs = past_the_limit(rigs)
    assert bitwise(outs[1], outs[0]) and bitwise(outs[2], outs[0])
    r.load(r.c, 0)
    r.d.train_step(r.s, r.a, r.R, r.adv, r.c.M, 1.0 / r.c.M, 1.0, ALPHA)
    assert bitwise(r.state(), outs[0])


@pytest.mark.parametrize("name", ["W515-33", "W515-257"])
def test_per_layer_path_is_repeatable_on_the_reference_trunk(rigs, name):
    """Mode 0 at 515 inputs on the 500 / 300 trunk (column sums of more than 256 columns: several row blocks at every M; 257 rows: several row splits of the filter
    gradients): two steps from the same state give bitwise equal parameters, Adam slots and losses."""
    r = rigs(name, 0)
    c, d = r.c, r.d
    outs = []
    for _ in range(2):
        r.reset()
        d.train_step(r.s, r.a, r.R, r.adv, c.M, 1.0 / c.M, 1.0, ALPHA)
        outs.append(r.state())
    assert not d.fused_ok() and bitwise(outs[1], outs[0])
    check_adam(r, name + " mode 0 (per-layer)")


@pytest.mark.parametrize("mode", [0, 1])
def test_tables_of_2_gib_are_refused_before_any_launch(rigs, mode):
    """n_rows x din x 4 >= 2^31 with a small real allocation: MI_ERR_SHAPE, and neither the gradient buffer nor the parameters are touched.  (Mode 0: on the
    reference-width engine, whose fused kernels take the same 32-bit offsets.)"""
    from mi355.ppo_device import PpoDevice
    L = milib.get()
    if mode == 1:
        r = rigs("W515-33", 1)
        c, d, own = r.c, r.d, False
    else:
        c = narrow_case("REF67")
        d, own = PpoDevice(c.input_dim, c.A, c.low, c.high, pc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE, hidden=c.hidden, max_batch=64), True
        d.load_params(c.theta, pc.old_names(c.theta_old))
    try:
        din, M = c.input_dim, 8
        n_rows = -(-(1 << 31) // (din * 4))
        assert n_rows * din * 4 >= 1 << 31 and (n_rows - 1) * din * 4 < 1 << 31
        s = torch.zeros(16, din, device=d.device)
        a, z = torch.zeros(16, c.A, device=d.device), torch.zeros(16, device=d.device)
        rows = torch.zeros(M, dtype=torch.int32, device=d.device)
        d.grads.fill_(-777.0)
        before = [d.params.clone(), d.adam_m.clone(), d.adam_v.clone()]
        p, st = milib.ptr, d.stream()
        rc = L.cdll.mi_ppo_train_step_idx(d.handle, st, p(s), p(a), p(z), p(z), None, p(rows), n_rows, M, 1.0 / M, 1.0, float(ALPHA), 0.9, 0.999, 1e-8)
        assert rc == -2, (rc, L.cdll.mi_last_error())
        assert b"2 GiB" in L.cdll.mi_last_error()
        rc = L.cdll.mi_ppo_train_step_vclip(d.handle, None, st, p(s), p(a), p(z), p(z), None, p(z), INF, p(rows), n_rows, M, 1.0 / M, 1.0, 0, float(ALPHA), 0.9, 0.999, 1e-8)
        assert rc == -2, rc
        stats = torch.full((9,), -777.0, dtype=torch.float64, device=d.device)
        scratch = torch.zeros(d.stats_scratch_doubles(M), dtype=torch.float64, device=d.device)
        rc = L.cdll.mi_ppo_update_stats_idx(d.handle, st, p(s), p(a), p(z), p(z), p(rows), n_rows, M, 0, p(scratch), p(stats), None, None)
        assert rc == -2, rc
        torch.cuda.synchronize()
        assert bool((d.grads == -777.0).all()) and bool((stats == -777.0).all()) and bitwise([d.params, d.adam_m, d.adam_v], before)
        # one row fewer is a table the kernels take (the rows named are inside the real allocation)
        rc = L.cdll.mi_ppo_update_stats_idx(d.handle, st, p(s), p(a), p(z), p(z), p(rows), n_rows - 1, M, 0, p(scratch), p(stats), None, None)
        torch.cuda.synchronize()
        assert rc == 0 and float(stats[0]) == M
        d.grads.zero_()
    finally:
        if own:
            d.close()


# ---------------------------------------------------------------------------------------------------------------------------------------- 5
Z_WIDE, K_MEAS, SRC = 100, 3, (4, 6, 3)


@pytest.fixture(scope="module")
def mlp_vae(tmp_path_factory):
    from vae.models import MlpVAE
    rng = np.random.RandomState(21)
    p = vo.init_mlp_vae_params(3, z_dim=Z_WIDE, source_shape=SRC, target_shape=SRC, encoder_sizes=(36,), decoder_sizes=(8,))
    for k in p:
        if k.endswith("bias"):
            p[k] = (0.05 * rng.standard_normal(p[k].shape)).astype(np.float32)
    v = MlpVAE(np.array(SRC), encoder_sizes=(36,), decoder_sizes=(8,), z_dim=Z_WIDE, model_dir=str(tmp_path_factory.mktemp("wide_vae")), precision="fp32", training=False)
    v.set_weights(p)
    v.init_session(init_logging=False)
    return v


def env_inputs(rng, n):
    frames = rng.randint(0, 256, (n,) + SRC, dtype=np.uint8)
    meas = np.stack([rng.uniform(-1, 1, n), rng.uniform(0, 1, n), rng.uniform(0, 30, n)], axis=1)
    return frames, meas, rng.standard_normal((n, 2)).astype(np.float32)


def collect(buf, rng, continuous):
    """Every lane steps `horizon` times; the continuous buffer's lane 1 reports done at its step 2 and goes on."""
    E, T = buf.num_envs, buf.horizon
    buf.reset()
    for t in range(T):
        f, ms, nz = env_inputs(rng, E)
        buf.step(f, ms, noise=nz)
        dones = np.zeros(E, bool)
        if continuous and t == 1:
            dones[1] = True
        buf.outcome(rng.uniform(0, 1, E), dones)
    f, ms, _ = env_inputs(rng, E)
    if continuous:
        need = buf.rows.needs_bootstrap()
        buf.bootstrap(f[need], ms[need])
    else:
        buf.bootstrap(f, ms)
    return buf.rows.valid_rows()


def buffer_class(continuous):
    import rollout
    return rollout.ContinuousRolloutBuffer if continuous else rollout.RolloutBuffer


@pytest.mark.parametrize("E,T", [(3, 5), (5, 20)])
@pytest.mark.parametrize("continuous", [False, True], ids=["RolloutBuffer", "ContinuousRolloutBuffer"])
def test_buffer_update_is_the_host_loop_of_fused_steps(mlp_vae, tmp_path, continuous, E, T):
    """With ppo.set_wide_inputs(): update() leaves parameters, Adam slots and theta_old bitwise those of a twin policy driven by hand -- the log pi_old cache over the
    table, then one train_step_idx per shuffled minibatch on the buffer's tables."""
    seed, epochs, batch = 5, 2, 8
    _, m_a = make_pair(tmp_path / "a", input_dim=Z_WIDE + K_MEAS)
    _, m_b = make_pair(tmp_path / "b", input_dim=Z_WIDE + K_MEAS)
    for m in (m_a, m_b):
        assert not m.dev.fused_ok()
        m.set_wide_inputs()
        assert m.dev.fused_ok() and m.dev.engine_wide_inputs() == 1
    buf = buffer_class(continuous)(mlp_vae, m_a, E, T, seed=3)
    valid = collect(buf, np.random.RandomState(71 + E), continuous)
    assert len(valid) == E * T
    np.random.seed(seed)
    out = buf.update(num_epochs=epochs, batch_size=batch)
    n_steps = epochs * -(-len(valid) // batch)
    assert len(out["losses"]) == n_steps and all(np.isfinite(list(rec.values())).all() for rec in out["losses"])
    # the twin
    d = m_b.dev
    m_b.update_old_policy()
    lp = torch.zeros(buf.n_table_rows, device=d.device)
    d.logp_old(buf.states, buf.actions, buf.n_table_rows, lp)
    assert torch.equal(lp[torch.from_numpy(valid).to(d.device).long()].view(torch.int32), buf.logp_old[torch.from_numpy(valid).to(d.device).long()].view(torch.int32))
    np.random.seed(seed)
    b1, b2 = np.float32(0.9), np.float32(0.999)
    for _ in range(epochs):
        idx = np.arange(len(valid))
        np.random.shuffle(idx)
        perm = torch.from_numpy(valid[idx]).to(d.device)
        for i in range(0, len(valid), batch):
            mb = perm[i:i + batch]
            n = int(mb.numel())
            d.train_step_idx(buf.states, buf.actions, buf.returns, buf.advantages, lp, mb, n, 1.0 / n, 1.0, _adam_alpha(m_b.current_learning_rate(), b1, b2), 0.9, 0.999, 1e-8)
            b1, b2 = np.float32(b1 * np.float32(0.9)), np.float32(b2 * np.float32(0.999))
    assert bitwise(flat_state(m_a), flat_state(m_b))
    assert not torch.equal(m_a.dev.params, m_a.dev.params_old)


@pytest.mark.parametrize("continuous", [False, True], ids=["RolloutBuffer", "ContinuousRolloutBuffer"])
def test_buffer_diagnostics_value_clip_and_kl_penalty(mlp_vae, tmp_path, continuous):
    """Without the setting update_with_diagnostics(), value clipping and the KL penalty raise the ValueError they raise today (now naming the setting); with it the
    update runs and returns its keys."""
    E, T = 3, 5
    _, m = make_pair(tmp_path / "m", input_dim=Z_WIDE + K_MEAS)
    buf = buffer_class(continuous)(mlp_vae, m, E, T, seed=3)
    collect(buf, np.random.RandomState(9), continuous)
    before = flat_state(m)
    with pytest.raises(ValueError, match=r"cached log pi_old.*\(more than 96 inputs: PPO\.set_wide_inputs\(\)\)"):
        buf.update_with_diagnostics(num_epochs=1, batch_size=8)
    m.set_value_clip(0.2)
    with pytest.raises(ValueError, match=r"value clipping.*PPO\.set_wide_inputs\(\)"):
        buf.update(num_epochs=1, batch_size=8)
    m.set_value_clip(None)
    m.set_kl_penalty(0.5, target=0.01)
    with pytest.raises(ValueError, match=r"KL penalty.*PPO\.set_wide_inputs\(\)"):
        buf.update(num_epochs=1, batch_size=8)
    assert bitwise(flat_state(m), before)
    m.set_wide_inputs()
    m.set_value_clip(0.2)
    np.random.seed(3)
    out = buf.update_with_diagnostics(num_epochs=2, batch_size=8)
    assert out["epochs_run"] == 2 and len(out["epochs"]) == 2 and len(out["losses"]) == 2 * 2
    for e in out["epochs"]:
        for k in ("samples", "approx_kl", "clip_fraction", "ratio_mean", "value_mse", "explained_variance", "value_clip_fraction", "value_loss_clipped",
                  "value_grad_zero_fraction"):
            assert k in e and np.isfinite(e[k]), (k, e)
        assert e["samples"] == E * T
    for k in ("kl", "kl_coef", "kl_coef_next", "kl_adapted"):
        assert k in out, k
    assert out["kl_coef"] == 0.5 and np.isfinite(out["kl"]["kl"]) and out["kl"]["kl"] >= 0 and all("kl" in rec and "kl_penalty" in rec for rec in out["losses"])
    assert not bitwise(flat_state(m), before)


def test_batched_rollout_step_at_103_inputs(mlp_vae, tmp_path):
    """BatchedRolloutStep at n = 3 within 1e-5 of vae.encode + ppo.predict, with the setting on (the step kernels split K = din themselves)."""
    from rollout import BatchedRolloutStep
    _, m = make_pair(tmp_path / "m", input_dim=Z_WIDE + K_MEAS)
    m.set_wide_inputs()
    step = BatchedRolloutStep(mlp_vae, m, 3, seed=3)
    f, ms, _ = env_inputs(np.random.RandomState(13), 3)
    a, v, states = step(f, ms, greedy=True)
    for e in range(3):
        z = mlp_vae.encode([f[e].astype(np.float32) / 255.0])[0]
        a2, v2 = m.predict(np.append(z, ms[e]), greedy=True)
        assert np.allclose(states[e, :Z_WIDE], z, rtol=1e-5, atol=1e-5), e
        assert np.allclose(a[e], np.asarray(a2).reshape(-1), rtol=1e-5, atol=1e-5) and float(v[e]) == pytest.approx(float(np.asarray(v2).reshape(-1)[0]), rel=1e-5, abs=1e-5), e
