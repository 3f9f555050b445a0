"""The PPO engine (PpoDevice / csrc/ppo_engine.hip, ppo_fused.hip, ppo_ops.hip) against the float64 oracle at shapes other than the reference's 67 -> 500 / 300 -> 2:
  A  1, 3 and 8 actions on the reference trunk: the PF_MAX_ACT instantiations of the head / loss, predict, log pi_old and statistics kernels, and A = 1, which
     runs the <2> heads everywhere but in the step;
  B  trunks (5, (36, 20)), (96, (132, 320)), (40, (100, 44)): one k-step and H2 < 32, the upper limits kin = 96 / H2 = 320, partial tiles everywhere;
  C  (100, (64, 64)) and (67, (64, 324)): kin = 104 and H2 = 324 are outside the fused kernels' range, the per-layer path runs.
Problems and references: tests/ppo_shape_cases.py (conditions on the reference: tests/test_ppo_shape_cases_host.py).  Bounds are the project's: fp32 1e-4 relative
(abs 1e-6) on loss scalars, 2e-4 of each tensor's max on gradients, rtol 1e-4 / atol 1e-5 on actions and values (tests/test_c_c3_ppo_gpu.py); bf16x3 1e-4 on loss
scalars and max(1e-3, 4 x the fp32 oracle's own distance from float64) on gradients (tests/test_j_ppo_bf16x3_gpu.py); per-row log pi 1e-4 of max |log pi| and the
statistics' rule of tests/test_p_rollout_diagnostics_gpu.py.  Every test prints the worst figure it saw next to its bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ppo_shape_cases as pc  # noqa: E402
from oracle import vae_oracle as vo  # noqa: E402
from mi355 import lib as milib  # noqa: E402
from ppo import _adam_alpha  # noqa: E402

LR = 1e-4
ALPHA = _adam_alpha(LR, 0.9, 0.999)
SMALL = [k for k, v in pc.ENGINE_CASES.items() if v[3] <= 256]                       # the in-kernel Adam needs the whole minibatch in one wave
SMALL_FUSED = [k for k in SMALL if k in pc.FUSED_CASES]
SHAPES = sorted({(v[0], v[1], v[2]) for v in pc.ENGINE_CASES.values()})
X3_LOSS_REL, X3_GRAD_FLOOR, X3_GRAD_FACTOR = 1e-4, 1e-3, 4.0


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


class Rig:
    """One engine with one case's parameters and samples on the device."""

    def __init__(self, name, precision):
        from mi355.ppo_device import PpoDevice
        self.c = c = pc.engine_case(name)
        self.fused = name in pc.FUSED_CASES
        self.d = d = PpoDevice(c.input_dim, c.A, c.low, c.high, pc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE, hidden=c.hidden, max_batch=320, precision=precision)
        assert d.fused_ok() == self.fused and d.kin == (c.input_dim + 7) // 8 * 8
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(d.device)      # noqa: E731
        self.s, self.a, self.R, self.adv = up(c.s), up(c.a), up(c.R), up(c.adv)
        self.reset()

    def reset(self):
        """theta, theta_old as the case has them; optimiser state and gradient buffer zero (the per-layer path accumulates into the gradient buffer)."""
        d = self.d
        d.load_params(self.c.theta, pc.old_names(self.c.theta_old))
        d.adam_m.zero_(); d.adam_v.zero_(); d.grads.zero_()

    def used(self):
        used = torch.zeros(self.d.n_flat, dtype=torch.bool, device=self.d.device)
        for _, (o_, s_) in self.d.layout.items():
            used[o_:o_ + s_] = True
        return used


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(name, precision="fp32"):
        if (name, precision) not in made:
            made[(name, precision)] = Rig(name, precision)
        r = made[(name, precision)]
        r.reset()
        return r
    yield get
    for r in made.values():
        r.d.close()


_G32 = {}


def fp32_oracle_distance(name):
    """Each gradient's distance of the float32 CPU oracle from float64, of its tensor max (the yardstick of the bf16x3 bound)."""
    if name not in _G32:
        c = pc.engine_case(name)
        g32 = pc.losses_and_grads(c.theta, c.theta_old, c.s, c.a, c.R, c.adv, c.low, c.high, dtype=torch.float32)[4]
        _G32[name] = {k: rel_err(g32[k], c.grads[k]) for k in c.grads}
    return _G32[name]


def check_losses(L, c, rel, tag):
    worst = 0.0
    for got, key in zip(L[:5], pc.LOSS_KEYS):
        worst = max(worst, abs(float(got) - c.scal[key]) / max(abs(c.scal[key]), 1e-30))
        assert float(got) == pytest.approx(c.scal[key], rel=rel, abs=pc.LOSS_ABS), (tag, key, float(got), c.scal[key])
    return worst


def grad_bounds(name, precision, grads):
    if precision == "fp32":
        return {k: pc.GRAD_REL for k in grads}
    d32 = fp32_oracle_distance(name)
    return {k: max(X3_GRAD_FLOOR, X3_GRAD_FACTOR * d32[k]) for k in grads}


def modes(names):
    return [(n, "fp32") for n in names] + [(n, "bf16x3") for n in names if n in pc.FUSED_CASES]


@pytest.mark.parametrize("name,precision", modes(list(pc.ENGINE_CASES)))
def test_gradient_pass_against_float64(rigs, name, precision):
    """forward_backward: five loss scalars, 13 gradients; fused path: the action-mean and std entries of the losses buffer, and a second pass over a gradient
    buffer full of 4.25 that is bitwise the first on every tensor's range (the pass stores, it does not accumulate)."""
    r = rigs(name, precision)
    c, d = r.c, r.d
    assert d.engine_precision() == (milib.MI_F32 if precision == "fp32" else milib.MI_BF16X3)
    d.forward_backward(r.s, r.a, r.R, r.adv, c.M, 1.0 / c.M, 1.0)
    L = d.losses.cpu().numpy().astype(np.float64)
    worst_l = check_losses(L, c, pc.LOSS_REL if precision == "fp32" else X3_LOSS_REL, name)
    g = d.export_grads()
    bound = grad_bounds(name, precision, c.grads)
    err = {k: rel_err(g[k], c.grads[k]) for k in c.grads}
    k_w = max(err, key=lambda k: err[k] / bound[k])
    print("\n%s %s: loss scalars %.2e (bound 1e-4), worst gradient %.2e of max (bound %.1e, %s)" % (name, precision, worst_l, err[k_w], bound[k_w], k_w))
    bad = {k: (err[k], bound[k]) for k in err if err[k] > bound[k]}
    assert not bad, bad
    if not r.fused:
        return
    A = c.A
    assert L.shape == (5 + 2 * A,)
    assert np.allclose(L[5:5 + A], c.mean.mean(0), rtol=pc.ACT_RTOL, atol=pc.ACT_ATOL), (L[5:5 + A], c.mean.mean(0))
    assert np.allclose(L[5 + A:], np.exp(c.theta["policy/action_logstd"].astype(np.float64)), rtol=1e-6), L[5 + A:]
    first = d.grads.clone()
    d.grads.fill_(4.25)
    d.losses.fill_(-3.0)
    d.forward_backward(r.s, r.a, r.R, r.adv, c.M, 1.0 / c.M, 1.0)
    used = r.used()
    assert torch.equal(d.grads[used].view(torch.int32), first[used].view(torch.int32))
    assert np.array_equal(d.losses.cpu().numpy().astype(np.float64), L)


@pytest.mark.parametrize("name,precision", modes(SMALL))
def test_train_step_against_adam_on_reference_gradients(rigs, name, precision):
    """train_step (fused: Adam inside the gradient kernels; per-layer: gradient pass + flat Adam): parameters against oracle.vae_oracle.AdamTF on the float64
    reference's gradients, as tests/test_c_c3_ppo_gpu.py::test_fused_step_gradients_update_and_cache_match_oracle checks them."""
    r = rigs(name, precision)
    c, d = r.c, r.d
    before = {k: v.copy() for k, v in c.theta.items()}
    want = {k: v.copy() for k, v in before.items()}
    grads = {k: v.astype(np.float32) for k, v in c.grads.items()}
    vo.AdamTF({k: v.shape for k, v in before.items()}).step(want, grads, LR)
    d.train_step(r.s, r.a, r.R, r.adv, c.M, 1.0 / c.M, 1.0, ALPHA)
    got = d.export_params()
    worst = 0.0
    for k in want:
        sig = np.abs(grads[k]) > 1e-6                     # where Adam's first step is +-lr regardless of rounding
        assert sig.any(), k
        worst = max(worst, float(np.abs(got[k][sig] - want[k][sig]).max()))
        assert np.allclose(got[k][sig], want[k][sig], rtol=0, atol=2e-6), (k, float(np.abs(got[k][sig] - want[k][sig]).max()))
        assert np.abs(got[k] - before[k]).max() <= 1.01e-4 + 1e-9, k
    L = d.losses.cpu().numpy().astype(np.float64)
    worst_l = check_losses(L, c, 1e-4, name)                 # the step's own loss scalars, in both precisions
    print("\n%s %s: parameters after the step, worst |diff| %.2e (bound 2e-6); loss scalars %.2e (bound 1e-4)" % (name, precision, worst, worst_l))


@pytest.mark.parametrize("name", SMALL_FUSED)
def test_train_step_from_the_cached_log_pi_old(rigs, name):
    """The step from the cached log pi_old (d.logp_old, the old policy's forward pass skipped) against the step that evaluates the old policy itself: the same
    parameters within atol 1e-7, the bound of tests/test_c_c3_ppo_gpu.py::test_fused_step_gradients_update_and_cache_match_oracle (3).

    This test found that bound missed at three and eight actions and on the (96, (132, 320)) trunk: worst |parameter diff| A3-33 1.04e-7, A3-77 3.17e-7, A8-33 9.13e-7,
    A8-77 5.33e-7, B96-33 1.49e-7, B96-77 3.02e-7 (A1, B5, B40: <= 3.0e-8).  The step then evaluated log pi_old in another order and with other exp / log / tanh than
    the kernel that fills the cache, so the two differed by an ulp of log pi_old (2.4e-7 .. 9.5e-7 at |log pi| ~ 3 .. 12), and Adam's first step lr g / (|g| + 3.2e-7)
    multiplies what that does to a gradient near zero by 316.  ppo_head_loss_kernel now spells the old policy's log-probability as ppo_predict_head_kernel does
    (csrc/ppo_fused.hip); the figures since are in profiles/r16_ppo_shapes.md."""
    r = rigs(name)
    c, d = r.c, r.d
    d.train_step(r.s, r.a, r.R, r.adv, c.M, 1.0 / c.M, 1.0, ALPHA)
    got = d.export_params()
    lp = torch.full((c.M,), float("nan"), device=d.device)
    r.reset()
    d.logp_old(r.s, r.a, c.M, lp)
    d.train_step(r.s, r.a, r.R, r.adv, c.M, 1.0 / c.M, 1.0, ALPHA, logp_old=lp)
    got2 = d.export_params()
    diff = {k: float(np.abs(got2[k] - got[k]).max()) for k in got}
    k_w = max(diff, key=diff.get)
    print("\n%s: cached log pi_old against the in-step old policy, worst |parameter diff| %.3e (%s; bound 1e-7)" % (name, diff[k_w], k_w))
    assert any(not np.array_equal(got[k], c.theta[k]) for k in got)
    for k in got:
        assert np.allclose(got2[k], got[k], rtol=0, atol=1e-7), (k, diff[k])


@pytest.mark.parametrize("name", SMALL_FUSED)
def test_train_step_idx_on_a_permuted_table_is_the_gathered_step(rigs, name):
    """Sample i sits in row pos[i] of tables of M + 7 rows (the other rows hold other finite numbers): train_step_idx on pos is bitwise train_step on the samples."""
    r = rigs(name)
    c, d = r.c, r.d
    M, T = c.M, c.M + 7
    rng = np.random.RandomState(M + c.A)
    pos = rng.permutation(T)[:M].astype(np.int32)

    def table(x):
        t = rng.uniform(-0.5, 0.5, (T,) + x.shape[1:]).astype(np.float32)
        t[pos] = x
        return torch.from_numpy(t).to(d.device)
    d.train_step(r.s, r.a, r.R, r.adv, M, 1.0 / M, 1.0, ALPHA)
    p0, l0 = d.params.clone(), d.losses.clone()
    assert not torch.equal(p0, torch.from_numpy(d._to_flat(c.theta)).to(d.device))
    r.reset()
    d.train_step_idx(table(c.s), table(c.a), table(c.R), table(c.adv), None, torch.from_numpy(pos).to(d.device), M, 1.0 / M, 1.0, ALPHA)
    assert torch.equal(d.params.view(torch.int32), p0.view(torch.int32)), float((d.params - p0).abs().max())
    assert torch.equal(d.losses.view(torch.int32), l0.view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%dx%d" % (s[0], s[1], s[2][0], s[2][1]))
def test_predict_sampled_and_greedy(rigs, shape):
    """M = 1, 8 (a wave per sample), 9, 33 (8 threads per sample): actions (noise past the bounds on both sides of every action index), values, the action_mean table."""
    name = next(k for k, v in pc.ENGINE_CASES.items() if (v[0], v[1], v[2]) == shape)
    r = rigs(name)
    c, d = r.c, r.d
    worst_a = worst_v = 0.0
    for M in (1, 8, 9, 33):
        p = pc.predict_inputs(c, M)
        if M >= 8:
            assert p["sides"]["low"].all() and p["sides"]["high"].all() and p["sides"]["inside"]
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
            assert (a[:M] >= c.low).all() and (a[:M] <= c.high).all()
            assert np.all(a[M:] == -777.0) and np.all(v[M:] == -777.0) and np.all(mean[M:] == -777.0)      # rows past M are nobody's
    print("\n%s: worst |action diff| %.2e, |value diff| %.2e (rtol 1e-4, atol 1e-5)" % (shape, worst_a, worst_v))


@pytest.mark.parametrize("name", pc.FUSED_CASES)
def test_logp_old_into_a_poisoned_buffer(rigs, name):
    """log pi_old of the samples under theta_old: 1e-4 of max |log pi| against float64, rows past M not written."""
    r = rigs(name)
    c, d = r.c, r.d
    lp = torch.full((c.M + 3,), float("nan"), device=d.device)
    d.logp_old(r.s, r.a, c.M, lp)
    got = lp.cpu().numpy()
    assert np.isnan(got[c.M:]).all() and np.isfinite(got[:c.M]).all()
    err = np.abs(got[:c.M] - c.logp_old).max() / np.abs(c.logp_old).max()
    print("\n%s: log pi_old, max |diff| / max |log pi| = %.2e (bound 1e-4)" % (name, err))
    assert err <= 1e-4, err


@pytest.mark.parametrize("name", pc.FUSED_CASES)
def test_update_statistics_against_float64(rigs, name):
    """update_stats over a permuted row table against the float64 statistics of tests/test_p_rollout_diagnostics_gpu.py (its helper, its bound: 1e-4 relative, or 4 x
    the distance of the fp32 torch-CPU evaluation where that is more; no sample is near the threshold, so the clipped count is exact)."""
    from mi355.ppo_device import N_STATS, update_stats_summary
    from test_p_rollout_diagnostics_gpu import STAT_KEYS, float64_statistics
    r = rigs(name)
    c, d = r.c, r.d
    M, T = c.M, c.M + 7
    rng = np.random.RandomState(3 * M + c.A)
    pos = rng.permutation(T)[:M].astype(np.int32)
    stats = torch.full((N_STATS,), -777.0, dtype=torch.float64, device=d.device)
    scratch = torch.zeros(d.stats_scratch_doubles(M), dtype=torch.float64, device=d.device)

    def table(x, fill):
        t = np.full((T,) + x.shape[1:], fill, np.float32)
        t[pos] = x
        return torch.from_numpy(t).to(d.device)
    rows = torch.from_numpy(pos).to(d.device)
    s_t, a_t, R_t = table(c.s, 0.25), table(c.a, float("nan")), table(c.R, float("nan"))      # (layer 1 reads a few entries of the row behind a named one: finite)
    lpo_t = torch.full((T,), float("nan"), device=d.device)
    lp = torch.empty(M, device=d.device)
    d.logp_old(r.s, r.a, M, lp)
    lpo_t[rows.long()] = lp
    lp_new, v_new = torch.full((T,), -777.0, device=d.device), torch.full((T,), -777.0, device=d.device)
    state = [x.clone() for x in (d.params, d.params_old, d.adam_m, d.adam_v, d.grads)]
    d.update_stats(s_t, a_t, R_t, lpo_t, rows, M, stats, scratch, logp_new_out=lp_new, value_out=v_new)
    got = update_stats_summary(stats.cpu().numpy())
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(state, (d.params, d.params_old, d.adam_m, d.adam_v, d.grads)))
    want, want32, lp64, near = float64_statistics(c.theta, pc.old_names(c.theta_old), c.s, c.a, c.R, c.low, c.high, eps=pc.EPS)
    assert near == 0 and np.allclose(lp64, c.logp, rtol=1e-12, atol=1e-12)
    other = np.setdiff1d(np.arange(T), pos)
    lpn, vn = lp_new.cpu().numpy(), v_new.cpu().numpy()
    assert np.all(lpn[other] == -777.0) and np.all(vn[other] == -777.0)
    err_lp = np.abs(lpn[pos] - lp64).max() / np.abs(lp64).max()
    assert err_lp <= 1e-4, err_lp
    assert np.allclose(vn[pos], c.value, rtol=pc.ACT_RTOL, atol=pc.ACT_ATOL)
    assert got["samples"] == M == want["samples"] and got["clip_fraction"] == want["clip_fraction"] and 0 < want["clip_fraction"] < 1
    print("\n%s: per-row log pi %.2e of max (bound 1e-4)" % (name, err_lp))
    for k in STAT_KEYS:
        dist, d32 = abs(got[k] - want[k]) / abs(want[k]), abs(want32[k] - want[k]) / abs(want[k])
        tol = max(1e-4, 4 * d32)
        print("  %-20s device %.2e, fp32 torch-CPU %.2e from float64 (relative); bound %.1e" % (k, dist, d32, tol))
        assert dist <= tol, (k, got[k], want[k], dist, tol)


@pytest.mark.parametrize("name", pc.PER_LAYER_CASES)
def test_per_layer_shapes_refuse_what_only_the_fused_kernels_do(rigs, name):
    """No value check: log pi_old, the update statistics and the in-kernel gather exist only as fused kernels.  An engine on the per-layer path refuses them with an
    error before anything is launched (the output buffers keep their contents); it does not compute them some other way."""
    from mi355.ppo_device import N_STATS
    r = rigs(name)
    c, d = r.c, r.d
    assert not r.fused
    M = c.M
    lp = torch.full((M + 3,), float("nan"), device=d.device)
    with pytest.raises(milib.MiError):
        d.logp_old(r.s, r.a, M, lp)
    rows = torch.arange(M, dtype=torch.int32, device=d.device)
    stats = torch.full((N_STATS,), -777.0, dtype=torch.float64, device=d.device)
    scratch = torch.zeros(d.stats_scratch_doubles(M), dtype=torch.float64, device=d.device)
    with pytest.raises(milib.MiError):
        d.update_stats(r.s, r.a, r.R, torch.zeros(M, device=d.device), rows, M, stats, scratch)
    before = d.params.clone()
    with pytest.raises(milib.MiError):
        d.train_step_idx(r.s, r.a, r.R, r.adv, None, rows, M, 1.0 / M, 1.0, ALPHA)
    torch.cuda.synchronize()
    assert bool(torch.isnan(lp).all()) and bool((stats == -777.0).all()) and torch.equal(d.params, before)


@pytest.mark.parametrize("name", pc.PER_LAYER_CASES)
def test_per_layer_shapes_refuse_the_split_mode(name):
    """mi_ppo_set_precision: the split-bf16 mode exists only as fused kernels; an engine on the per-layer path refuses it instead of training in fp32."""
    from mi355.ppo_device import PpoDevice
    c = pc.engine_case(name)
    with pytest.raises(milib.MiError):
        PpoDevice(c.input_dim, c.A, c.low, c.high, pc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE, hidden=c.hidden, max_batch=64, precision="bf16x3")
    d = PpoDevice(c.input_dim, c.A, c.low, c.high, pc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE, hidden=c.hidden, max_batch=64)
    assert not d.fused_ok() and d.engine_precision() == milib.MI_F32
    d.close()
