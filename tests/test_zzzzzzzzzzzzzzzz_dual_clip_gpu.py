"""Dual-clip PPO and the runtime loss coefficients on the GPU (mi_ppo_set_dual_clip, mi_ppo_set_loss_coefs, mi_ppo_dual_clip_stats, PPO.set_dual_clip,
PPO.set_loss_coefficients and the rollout buffers).

Problems: tests/dual_clip_cases.py -- planned rows (a target ratio and a sign of A per row, realised through the cached log pi_old) on 2 actions x 67 -> 500 / 300,
3 actions x 5 -> 36 / 20 and the wide 2 actions x 131 -> 36 / 20, M = 5 / 33 / 257, as contiguous tensors and through row_idx into tables of 2 M + 3 rows with NaN in
every row of every table that the index does not name.  The float64 reference is dual_clip_cases.reference (numpy; checked on the host against finite differences
and against the oracle's autograd).  Bounds are the step's own (tests/ppo_shape_cases.py, tests/test_j_ppo_bf16x3_gpu.py, tests/behaviour_cloning_cases.py).

The step that realises a planned ratio needs the cached log pi_old and, for its gradients, adam = 0: that is mi_ppo_train_step_vclip with eps_v = +inf (the plain
value loss bit for bit: tests/test_s_value_clip_gpu.py).  The per-layer loss kernel mi_ppo_loss_fwd_bwd takes no handle, so "the per-layer path refuses" is tested
where the handle is: mi_ppo_forward_backward / mi_ppo_train_step of an engine outside the fused range."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dual_clip_cases as dc  # noqa: E402
import ppo_shape_cases as pc  # noqa: E402
from rollout_gpu_common import bitwise, flat_state  # noqa: E402

C, INF, ALPHA = dc.C, float("inf"), 1e-4
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8
ADAM_ABS = 2e-6                                           # tests/behaviour_cloning_cases.py: parameters after Adam against TF-Adam on the device's gradients
X3_GRAD_FLOOR, X3_GRAD_FACTOR = 1e-3, 4.0                 # tests/test_j_ppo_bf16x3_gpu.py
N_DEMO = 3
ENTRIES = ("plain", "vclip", "kl", "demo")


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


class Problem:
    pass


class Rig:
    """One engine per (shape, precision) and its problems per (M, positive): contiguous tensors, the same samples as rows of NaN-padded tables."""

    def __init__(self, shape, precision):
        import torch
        from mi355.ppo_device import PpoDevice
        self.shape, self.precision = shape, precision
        self.din, self.A, self.hidden, _, _, self.wide = dc.SHAPES[shape]
        low, high = pc.bounds(self.A)
        self.d = PpoDevice(self.din, self.A, low, high, dc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE, hidden=self.hidden, max_batch=320, precision=precision,
                           wide_inputs=self.wide)
        assert self.d.fused_ok() and self.d.engine_dual_clip() == 0.0
        self.used = torch.zeros(self.d.n_flat, dtype=torch.bool, device=self.d.device)
        for _, (o_, s_) in self.d.layout.items():
            self.used[o_:o_ + s_] = True
        self.problems = {}

    def up(self, x):
        import torch
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.d.device)

    def restore(self, q, dual=None, fill=4.25):
        d = self.d
        for x, y in zip((d.params, d.adam_m, d.adam_v, d.params_old), q.state0 + [q.old]):
            x.copy_(y)
        d.grads.fill_(fill)
        d.set_max_grad_norm(None)
        d.set_dual_clip(dual)

    def problem(self, M, positive=False):
        import torch
        key = (M, positive)
        if key in self.problems:
            return self.problems[key]
        d = self.d
        q = Problem()
        q.M, q.c = M, dc.planned(self.shape, M, positive)
        c = q.c
        d.load_params(c.theta, pc.old_names(c.theta_old))
        d.adam_m.zero_(); d.adam_v.zero_()
        q.state0, q.old = [x.clone() for x in (d.params, d.adam_m, d.adam_v)], d.params_old.clone()
        q.s, q.a, q.R, q.adv, q.lp = self.up(c.s), self.up(c.a), self.up(c.R), self.up(c.adv), self.up(c.logp_old)
        q.v_old = torch.zeros(M, device=d.device)                                     # (read by the vclip entry at eps_v = inf: never clips)
        q.mean_old, scratch_lp = torch.empty(M, self.A, device=d.device), torch.empty(M, device=d.device)
        d.old_policy_cache(q.s, q.a, M, scratch_lp, q.mean_old)                       # the old policy's means for the KL entry (beta = 0 measures only)
        rng = np.random.RandomState(300 + M)
        q.demo_s, q.demo_a = self.up(0.5 * rng.standard_normal((N_DEMO, self.din))), self.up(np.clip(0.3 * rng.standard_normal((N_DEMO, self.A)), c.low, c.high))
        n = 2 * M + 3
        rows = rng.permutation(n)[:M].astype(np.int32)
        q.rows = torch.from_numpy(rows).to(d.device)
        idx = q.rows.long()
        q.tab = {}
        for name, x in (("s", q.s), ("a", q.a), ("R", q.R), ("adv", q.adv), ("lp", q.lp), ("v_old", q.v_old), ("mean_old", q.mean_old)):
            t = torch.full((n,) + tuple(x.shape[1:]), float("nan"), device=d.device)
            t[idx] = x
            q.tab[name] = t
        self.problems[key] = q
        return q

    def step(self, q, form="flat", entry="vclip", adam=True, comm=None):
        """One step from the state as it stands -> (params / m / v, losses, gradient buffer, du [M, A], dv [M]); always with the cached log pi_old."""
        d, M = self.d, q.M
        a = (1.0 / M, 1.0, ALPHA)
        t = (lambda k: getattr(q, k)) if form == "flat" else (lambda k: q.tab[k])
        rows = None if form == "flat" else q.rows
        four = (t("s"), t("a"), t("R"), t("adv"))
        if entry == "plain":
            assert adam
            if comm is not None:
                d.train_step_dp(comm, *four, t("lp"), rows, M, *a)
            elif form == "flat":
                d.train_step(*four, M, *a, logp_old=t("lp"))
            else:
                d.train_step_idx(*four, t("lp"), rows, M, *a)
        elif entry == "vclip":
            d.train_step_vclip(comm, *four, t("lp"), t("v_old"), INF, rows, M, *a, adam=adam)
        elif entry == "kl":
            d.train_step_kl(comm, *four, t("lp"), t("mean_old"), 0.0, rows, M, *a, adam=adam)
        else:
            d.train_step_demo(comm, *four, t("lp"), None, None, rows, M, q.demo_s, q.demo_a, None, N_DEMO, "nll", 0.5, 1.0 / N_DEMO, *a, adam=adam)
        return ([x.clone() for x in (d.params, d.adam_m, d.adam_v)], d.losses.clone(), d.grads.clone(), d.policy_head_grad[:M].clone(), d.value_head_grad[:M].clone())


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(shape, precision="fp32"):
        if (shape, precision) not in made:
            made[(shape, precision)] = Rig(shape, precision)
        return made[(shape, precision)]
    yield get
    for r in made.values():
        r.d.close()


@pytest.fixture(scope="module")
def recording_comm():
    from mi355 import lib as milib
    L = milib.get()
    hcomm, log = ctypes.c_void_p(), np.zeros((256, 4), np.int64)
    L.mi_comm_init_recording(ctypes.addressof(hcomm), 0, 1, log.ctypes.data, 256)
    yield hcomm
    L.mi_comm_destroy(hcomm)


GRID = [(s, p, M) for s in dc.SHAPES for p in ("fp32", "bf16x3") for M in dc.MS]
_REF = {}


def float64_reference(q):
    key = (q.c.shape, q.M)
    if key not in _REF:
        c = q.c
        scal, g64, per = dc.reference(c.theta, c.s, c.a, c.R, c.adv, c.logp_old, c.low, c.high)
        _, g32, _ = dc.reference(c.theta, c.s, c.a, c.R, c.adv, c.logp_old, c.low, c.high, dtype=np.float32)
        assert np.array_equal(per["dual"], c.cls == dc.DUAL)
        _REF[key] = (scal, g64, per, {k: rel_err(g32[k], g64[k]) for k in g64})
    return _REF[key]


def same_step(x, y, what=(0, 1, 2)):
    return all(bitwise(x[i], y[i]) for i in what)


@pytest.mark.parametrize("form", ["flat", "idx"])
@pytest.mark.parametrize("shape,precision,M", GRID)
def test_the_planned_rows_against_float64(rigs, shape, precision, M, form):
    r = rigs(shape, precision)
    q, d = r.problem(M), r.d
    c = q.c
    scal, g64, per, d32 = float64_reference(q)
    r.restore(q, C)
    assert d.engine_dual_clip() == C
    params, losses, _, du, dv = r.step(q, form, adam=False)
    g = d.export_grads()
    L = losses.cpu().numpy().astype(np.float64)
    got = dict(policy_loss=L[0], value_loss=L[1], entropy_loss=L[2], loss=L[3], ratio_mean=L[4])
    terms = abs(scal["policy_loss"]) + abs(scal["value_loss"]) + abs(scal["entropy_loss"])
    print("\n%s %s M = %d %s:" % (shape, precision, M, form))
    for k in ("policy_loss", "value_loss", "entropy_loss", "ratio_mean"):
        print("  %-13s %.9g (float64 %.9g, rel %.2e)" % (k, got[k], scal[k], abs(got[k] - scal[k]) / abs(scal[k])))
    print("  %-13s %.9g (float64 %.9g, %.2e of the sum of its absolute terms)" % ("loss", got["loss"], scal["loss"], abs(got["loss"] - scal["loss"]) / terms))
    bound = {k: pc.GRAD_REL if precision == "fp32" else max(X3_GRAD_FLOOR, X3_GRAD_FACTOR * d32[k]) for k in dc.NAMES}
    err = {k: rel_err(g[k], g64[k]) for k in dc.NAMES}
    for k in dc.NAMES:
        print("  %-26s %.3e of max (bound %.1e)" % (k, err[k], bound[k]))
    for k in ("policy_loss", "value_loss", "entropy_loss", "ratio_mean"):
        assert got[k] == pytest.approx(scal[k], rel=1e-4), k
    assert abs(got["loss"] - scal["loss"]) <= 1e-4 * terms
    assert not {k: (err[k], bound[k]) for k in dc.NAMES if err[k] > bound[k]}
    # the per-sample gradient of the action-mean head: exactly 0.0 on every dual-clipped row (the KL penalty is off), flowing where the plan says so
    du = du.cpu().numpy()
    flowing = (c.cls == dc.NEG_FLOW) | (c.cls == dc.POS_LOW) | (c.cls == dc.POS_IN)
    assert (c.cls == dc.DUAL).any() and np.all(du[c.cls == dc.DUAL] == 0.0), du[c.cls == dc.DUAL]
    assert np.all(du[(c.cls == dc.NEG_LOW) | (c.cls == dc.POS_HIGH)] == 0.0) and np.all(np.abs(du[flowing]).max(axis=1) > 0.0)
    print("  du per sample: %.3e of max" % rel_err(du, per["du"]))
    assert rel_err(du, per["du"]) <= (pc.GRAD_REL if precision == "fp32" else 1e-3)
    assert bitwise(params, q.state0)                                                 # adam = 0 leaves the parameters and the optimiser state alone
    # the value side and the entropy term are not touched: bitwise the step with the setting off.  The policy side is.
    r.restore(q, None)
    _, losses_u, _, du_u, dv_u = r.step(q, form, adam=False)
    g_u = d.export_grads()
    for k in dc.VALUE_NET:
        assert np.array_equal(g[k].view(np.int32), g_u[k].view(np.int32)), k
    Lu, Lc = losses_u.cpu().numpy(), losses.cpu().numpy()
    assert Lc[1].tobytes() == Lu[1].tobytes() and Lc[2].tobytes() == Lu[2].tobytes() and Lc[4].tobytes() == Lu[4].tobytes() and bitwise(dv, dv_u)
    du_u = du_u.cpu().numpy()
    assert np.all(np.abs(du_u[c.cls == dc.DUAL]).max(axis=1) > 0.0) and np.array_equal(du_u[c.cls != dc.DUAL].view(np.int32), du[c.cls != dc.DUAL].view(np.int32))
    assert Lc[0] > Lu[0] and not np.array_equal(g["policy/action_mean/kernel"], g_u["policy/action_mean/kernel"])      # mean(s') > mean(s): c A > s on the dual-clipped rows
    # Adam: the parameters of the one-call step against TF-Adam in float64 on the device's own gradients
    r.restore(q, C)
    after = r.step(q, form, "plain")[0]
    got_p = d.export_params()
    worst = 0.0
    for k in dc.NAMES:
        gk = g[k].astype(np.float64)
        want = c.theta[k].astype(np.float64) - ALPHA * ((1 - B1) * gk) / (np.sqrt((1 - B2) * gk * gk) + ADAM_EPS)
        worst = max(worst, float(np.abs(got_p[k] - want).max()))
    print("  parameters after Adam: %.3e from TF-Adam on the device's gradients" % worst)
    assert worst <= ADAM_ABS and not bitwise(after[0], q.state0[0])
    r.restore(q)


@pytest.mark.parametrize("shape,precision,M", GRID)
def test_c_infinite_and_all_positive_rows_are_the_setting_off(rigs, recording_comm, shape, precision, M):
    """c = inf against the setting off on train_step / _idx / _dp / _vclip / _kl / _demo and on the adam = 0 gradient buffers (the cached forms and
    mi_ppo_forward_backward, which evaluates the old policy in the step); a finite c on rows that all have A > 0 likewise."""
    r = rigs(shape, precision)
    for q, c_on in ((r.problem(M), INF), (r.problem(M, positive=True), C)):
        for form in ("flat", "idx"):
            for entry, adam, comm in [(e, True, None) for e in ENTRIES] + [("plain", True, recording_comm), ("vclip", False, None), ("kl", False, None), ("demo", False, None)]:
                r.restore(q, None)
                want = r.step(q, form, entry, adam, comm)
                r.restore(q, c_on)
                got = r.step(q, form, entry, adam, comm)
                assert same_step(got, want, (0, 1, 2, 3, 4)), (shape, precision, M, c_on, form, entry, adam, comm is not None)
        d = r.d
        r.restore(q, None)
        d.forward_backward(q.s, q.a, q.R, q.adv, M, 1.0 / M, 1.0)
        want = (d.grads.clone(), d.losses.clone())
        assert bool((want[0][r.used] != 4.25).any())
        r.restore(q, c_on)
        d.forward_backward(q.s, q.a, q.R, q.adv, M, 1.0 / M, 1.0)
        assert bitwise(list(want), [d.grads, d.losses])
        r.restore(q)


@pytest.mark.parametrize("shape,precision,M", GRID)
def test_reproducible_rows_communicator_and_the_global_norm_route(rigs, recording_comm, shape, precision, M):
    import torch
    r = rigs(shape, precision)
    q, d = r.problem(M), r.d
    runs = {}
    for form in ("flat", "idx"):
        r.restore(q, C)
        runs[form] = r.step(q, form, "plain")
        r.restore(q, C)
        assert same_step(r.step(q, form, "plain"), runs[form], (0, 1, 2, 3, 4)), form      # two runs
    assert same_step(runs["idx"], runs["flat"], (0, 1, 3, 4))                        # row_idx against contiguous
    assert not bitwise(runs["flat"][0][0], q.state0[0])
    for form in ("flat", "idx"):
        # the recording communicator (the flat route at every M) against adam = 0 + mi_ppo_apply_adam
        r.restore(q, C)
        dp = r.step(q, form, "plain", comm=recording_comm)
        r.restore(q, C)
        r.step(q, form, "vclip", adam=False)
        d.apply_adam(ALPHA)
        assert bitwise([d.params, d.adam_m, d.adam_v], dp[0]) and bitwise(dp[1], runs[form][1]), form
        # clipping by the global norm: "gradient buffer x factor, then Adam"
        r.restore(q, C)
        d.set_max_grad_norm(0.5)
        clipped = r.step(q, form, "plain") + (d.grad_clip.clone(),)
        rec = clipped[5]
        assert rec[2].item() == 0.5 and 0.0 < rec[1].item() <= 1.0 and rec[0].item() > 0.0
        r.restore(q, C)
        r.step(q, form, "vclip", adam=False)
        d.grads.mul_(rec[1])
        d.apply_adam(ALPHA)
        assert bitwise([d.params, d.adam_m, d.adam_v], clipped[0]), (form, rec)
        assert not bool(clipped[2].any()) and torch.equal(clipped[1], runs[form][1])
    r.restore(q)


def test_the_per_layer_path_refuses():
    """An engine outside the fused range (padded input width 104 > 96) with the setting on: mi_ppo_forward_backward and mi_ppo_train_step return MI_ERR_SHAPE in
    front of the first launch -- the gradient buffer, the per-sample du / dv workspaces (8 sentinels and more behind every output) and the parameters survive."""
    import torch
    from mi355 import lib as milib
    from mi355.ppo_device import PpoDevice
    low, high = pc.bounds(3)
    d = PpoDevice(100, 3, low, high, pc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE, hidden=(64, 64), max_batch=32)
    assert not d.fused_ok()
    z = lambda *s: torch.zeros(*s, device=d.device)      # noqa: E731
    d.forward_backward(z(5, 100), z(5, 3), z(5), z(5), 5, 0.2, 1.0)                   # off: the per-layer pass runs
    d.set_dual_clip(C)                                                                # (setting it is allowed: the refusal is the step's)
    d.grads.fill_(4.25); d.workspace.view(torch.float32)[:] = 7.5                     # (the engine is closed below: nothing reads the workspace again)
    ws_before = d.workspace.clone()
    before = [x.clone() for x in (d.params, d.adam_m, d.adam_v)]
    with pytest.raises(milib.MiError, match=r"mi_ppo_forward_backward failed \(-2\).*dual clip is on.*no per-layer form"):
        d.forward_backward(z(5, 100), z(5, 3), z(5), z(5), 5, 0.2, 1.0)
    with pytest.raises(milib.MiError, match=r"mi_ppo_train_step failed \(-2\).*dual clip is on"):
        d.train_step(z(5, 100), z(5, 3), z(5), z(5), 5, 0.2, 1.0, ALPHA)
    torch.cuda.synchronize()
    assert bool((d.grads == 4.25).all()) and torch.equal(d.workspace, ws_before) and bitwise([d.params, d.adam_m, d.adam_v], before)
    d.close()


@pytest.mark.parametrize("shape,M", [(s, M) for s in dc.SHAPES for M in dc.MS])
def test_dual_clip_stats(rigs, shape, M):
    import torch
    from mi355.ppo_device import N_DUAL_CLIP_STATS, dual_clip_summary
    r = rigs(shape)
    q, d = r.problem(M), r.d
    c = q.c
    r.restore(q)
    n = q.tab["lp"].shape[0]
    f64 = lambda k: torch.zeros(k, dtype=torch.float64, device=d.device)      # noqa: E731
    lp_new = torch.full((n,), float("nan"), device=d.device)                         # log pi_theta: the float64 value rounded to fp32, at the named rows only
    lp_new[q.rows.long()] = r.up(c.logp64)
    rows = q.rows.cpu().numpy()
    assert d.dual_clip_scratch_doubles(M) == N_DUAL_CLIP_STATS * ((M + 255) // 256)

    def run(lp, lpo, adv, idx, m, stats, accumulate=False):
        scratch = torch.full((d.dual_clip_scratch_doubles(m),), -1.0, dtype=torch.float64, device=d.device)
        d.dual_clip_stats(lp, lpo, adv, idx, m, dc.EPS, C, stats, scratch, accumulate=accumulate)
        return stats.cpu().numpy()
    got = run(lp_new, q.tab["lp"], q.tab["adv"], q.rows, M, torch.full((N_DUAL_CLIP_STATS,), 7.0, dtype=torch.float64, device=d.device)).copy()
    want = dc.stats_reference(lp_new.cpu().numpy(), q.tab["lp"].cpu().numpy(), q.tab["adv"].cpu().numpy(), rows)
    print("\n%s M = %d: sums %s, numpy float64 %s" % (shape, M, got, want))
    neg = (c.cls == dc.DUAL) | (c.cls == dc.NEG_FLOW) | (c.cls == dc.NEG_LOW)
    assert got[0] == M and got[1] == neg.sum() and got[2] == (c.cls == dc.DUAL).sum()       # exact against the plan
    assert np.array_equal(got[:3], want[:3])
    assert abs(got[3] - want[3]) <= 1e-9 * abs(want[3]) and abs(got[4] - want[4]) <= 1e-9 * abs(want[4])
    assert run(lp_new, q.tab["lp"], q.tab["adv"], q.rows, M, f64(N_DUAL_CLIP_STATS)).tobytes() == got.tobytes()      # run to run
    # NaN in the rows that are not named changes nothing: the same samples as tables of exactly M rows
    dense = run(lp_new[q.rows.long()].contiguous(), q.lp, q.adv, torch.arange(M, dtype=torch.int32, device=d.device), M, f64(N_DUAL_CLIP_STATS))
    assert dense.tobytes() == got.tobytes()
    # two chunks with accumulate: the counts bitwise, the sums within 1e-12
    cut = max(1, M // 3)
    acc = f64(N_DUAL_CLIP_STATS)
    run(lp_new, q.tab["lp"], q.tab["adv"], q.rows[:cut].contiguous(), cut, acc)
    chunked = run(lp_new, q.tab["lp"], q.tab["adv"], q.rows[cut:].contiguous(), M - cut, acc, accumulate=True)
    assert chunked[:3].tobytes() == got[:3].tobytes() and np.all(np.abs(chunked[3:] - got[3:]) <= 1e-12 * np.abs(got[3:]))
    s = dual_clip_summary(got)
    assert s["dual_clip_fraction"] == (c.cls == dc.DUAL).mean() and s["negative_advantage_fraction"] == neg.mean()
    assert s["surrogate_mean"] == got[3] / M and s["surrogate_mean_unclipped"] == got[4] / M and s["surrogate_mean"] > s["surrogate_mean_unclipped"]
    # the counts say what the step does: the rows whose du it zeroes beyond those the plain step zeroes
    r.restore(q, C)
    du_c = r.step(q, "idx", adam=False)[3].cpu().numpy()
    r.restore(q, None)
    du_u = r.step(q, "idx", adam=False)[3].cpu().numpy()
    assert int(((du_c == 0.0).all(axis=1) & ~(du_u == 0.0).all(axis=1)).sum()) == int(got[2])
    # c = inf: no row is dual-clipped and both sums are the plain surrogate's
    scratch = f64(d.dual_clip_scratch_doubles(M))
    never = f64(N_DUAL_CLIP_STATS)
    d.dual_clip_stats(lp_new, q.tab["lp"], q.tab["adv"], q.rows, M, dc.EPS, INF, never, scratch)
    never = never.cpu().numpy()
    assert never[2] == 0.0 and never[3].tobytes() == never[4].tobytes() == got[4].tobytes()
    assert bitwise([d.params, d.adam_m, d.adam_v], q.state0)                         # nothing but scratch and stats is written
    r.restore(q)


def test_the_setters_on_a_live_engine(rigs):
    from mi355 import lib as milib
    r = rigs("A3")
    q, d = r.problem(33), r.d
    r.restore(q, C)
    for bad in (0.5, 1.0, -3.0, float("nan"), float("-inf")):
        with pytest.raises(milib.MiError, match=r"mi_ppo_set_dual_clip failed \(-1\): mi_ppo_set_dual_clip: c is 0"):
            d.L.mi_ppo_set_dual_clip(d.handle, bad)
        assert d.engine_dual_clip() == C, bad                                         # refused: the setting is what it was
        with pytest.raises(ValueError):
            d.set_dual_clip(bad)
    d.set_dual_clip(INF)
    assert d.engine_dual_clip() == INF
    d.set_dual_clip(None)
    assert d.engine_dual_clip() == 0.0
    want = tuple(float(np.float32(x)) for x in (dc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE))
    assert d.engine_loss_coefs() == want
    for bad in ((0.0, 1.0, 0.0), (-0.2, 1.0, 0.0), (float("inf"), 1.0, 0.0), (float("nan"), 1.0, 0.0), (0.2, -1.0, 0.0), (0.2, float("nan"), 0.0), (0.2, 1.0, -0.1),
                (0.2, 1.0, float("inf"))):
        with pytest.raises(milib.MiError, match=r"mi_ppo_set_loss_coefs failed \(-1\)"):
            d.L.mi_ppo_set_loss_coefs(d.handle, *bad)
        with pytest.raises(ValueError):
            d.set_loss_coefs(*bad)
        assert d.engine_loss_coefs() == want and (d.clip_eps, d.value_scale, d.entropy_scale) == (dc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE), bad
    r.restore(q)


@pytest.mark.parametrize("shape,M", [("A2", 33), ("A3", 257)])
def test_loss_coefficients_on_a_live_engine(rigs, shape, M):
    """Setting the constructed values leaves a step bitwise unchanged; after set_loss_coefs(0.1, 1.0, 0.0) a step and the statistics pass are bitwise those of a
    fresh engine created with those values and loaded with the same parameters and slots; the values survive ensure_batch's new engine."""
    import torch
    from mi355.ppo_device import N_STATS, PpoDevice
    r = rigs(shape)
    q, d = r.problem(M), r.d
    n = q.tab["lp"].shape[0]

    def observe(dev):
        stats = torch.zeros(N_STATS, dtype=torch.float64, device=dev.device)
        scratch = torch.zeros(dev.stats_scratch_doubles(M), dtype=torch.float64, device=dev.device)
        lp_out, v_out = torch.zeros(n, device=dev.device), torch.zeros(n, device=dev.device)
        dev.update_stats(q.tab["s"], q.tab["a"], q.tab["R"], q.tab["lp"], q.rows, M, stats, scratch, logp_new_out=lp_out, value_out=v_out)
        return [stats.clone(), lp_out, v_out]
    r.restore(q, C)
    want = r.step(q, "idx", "plain")
    r.restore(q, C)
    d.set_loss_coefs(dc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE)
    assert same_step(r.step(q, "idx", "plain"), want, (0, 1, 2, 3, 4))
    r.restore(q, C)
    stats_before = observe(d)
    d.set_loss_coefs(0.1, 1.0, 0.0)
    assert d.engine_loss_coefs() == (float(np.float32(0.1)), 1.0, 0.0)
    stats_live = observe(d)
    live = r.step(q, "idx", "plain")
    live_g = r.step(q, "flat", "vclip", adam=False)[2]
    assert stats_live[0][3].item() >= stats_before[0][3].item()                       # the clipped count cannot fall with the range (the planned 0.9 and 1.1 sit on 0.1 itself)
    assert not bitwise(live[0][0], want[0][0])
    fresh = PpoDevice(r.din, r.A, q.c.low, q.c.high, 0.1, 1.0, 0.0, hidden=r.hidden, max_batch=320, wide_inputs=r.wide)
    try:
        for x, y in zip((fresh.params, fresh.adam_m, fresh.adam_v, fresh.params_old), q.state0 + [q.old]):
            x.copy_(y)
        fresh.grads.fill_(4.25)
        fresh.set_dual_clip(C)
        assert bitwise(observe(fresh), stats_live)
        a = (1.0 / M, 1.0, ALPHA)
        fresh.train_step_idx(q.tab["s"], q.tab["a"], q.tab["R"], q.tab["adv"], q.tab["lp"], q.rows, M, *a)
        assert bitwise([fresh.params, fresh.adam_m, fresh.adam_v, fresh.losses], live[0] + [live[1]])
        fresh.train_step_vclip(None, q.s, q.a, q.R, q.adv, q.lp, q.v_old, INF, None, M, *a, adam=False)
        assert bitwise(fresh.grads, live_g)
    finally:
        fresh.close()
    # a new engine of this object (ensure_batch) is created with the live values and the live constant
    small = PpoDevice(r.din, r.A, q.c.low, q.c.high, dc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE, hidden=r.hidden, max_batch=8, wide_inputs=r.wide)
    try:
        small.set_loss_coefs(0.1, 1.0, 0.0)
        small.set_dual_clip(C)
        handle = small.handle
        small.ensure_batch(64)
        assert small.handle != handle and small.engine_loss_coefs() == (float(np.float32(0.1)), 1.0, 0.0) and small.engine_dual_clip() == C
    finally:
        small.close()
    d.set_loss_coefs(dc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE)                        # the rig goes back to its constructed values: the step is the first one again
    r.restore(q, C)
    assert same_step(r.step(q, "idx", "plain"), want, (0, 1, 2, 3, 4))
    r.restore(q)


def test_ppo_honours_both_settings(tmp_path, monkeypatch):
    """PPO.set_dual_clip before and after init_session(), the knob, PPO.set_loss_coefficients on a live model, and train_step() against a twin's device call."""
    import torch
    from rollout_gpu_common import make_pair
    monkeypatch.setenv("MI355_PPO_DUAL_CLIP", "2.5")
    _, m = make_pair(tmp_path / "a")
    assert m.dual_clip == 2.5 and m.dev.engine_dual_clip() == 2.5
    monkeypatch.delenv("MI355_PPO_DUAL_CLIP")
    m.set_dual_clip(1.01)
    assert m.dev.engine_dual_clip() == float(np.float32(1.01))
    m.set_loss_coefficients(epsilon=0.1, entropy_scale=0.0)
    assert (m.epsilon, m.value_scale, m.entropy_scale) == (0.1, 1.0, 0.0) and m.dev.engine_loss_coefs() == (float(np.float32(0.1)), 1.0, 0.0)
    with pytest.raises(ValueError, match="PPO.set_loss_coefficients"):
        m.set_loss_coefficients(epsilon=-1.0)
    assert m.dev.engine_loss_coefs() == (float(np.float32(0.1)), 1.0, 0.0)
    _, twin = make_pair(tmp_path / "b", epsilon=0.1, entropy_scale=0.0)
    twin.dev.set_dual_clip(1.01)
    assert bitwise(flat_state(m), flat_state(twin))
    # the old policy's log-stds are raised by 0.3 each: a sample within one sigma of its mean has r = e^0.6 exp(-z^2 (1 - e^-0.6) / 2) >= 1.27 per pair of
    # actions, so every row with A < 0 lies above c = 1.01 and is dual-clipped in both
    def widen_old(x):
        o_, s_ = x.dev.layout["policy/action_logstd"]
        x.dev.params_old[o_:o_ + s_] += 0.3
    widen_old(m); widen_old(twin)
    rng = np.random.RandomState(4)
    s, a = (0.5 * rng.standard_normal((33, 67))).astype(np.float32), np.clip(0.3 * rng.standard_normal((33, 2)), [-1, 0], [1, 1]).astype(np.float32)
    R, adv = rng.standard_normal(33).astype(np.float32), rng.standard_normal(33).astype(np.float32)
    out = m.train_step(s, a, R, adv)
    up = lambda x: torch.from_numpy(x).to(twin.dev.device)      # noqa: E731
    from ppo import _adam_alpha
    twin.dev.train_step(up(s), up(a), up(R), up(adv), 33, 1.0 / 33, 1.0, _adam_alpha(twin.current_learning_rate(), np.float32(B1), np.float32(B2)), B1, B2, ADAM_EPS)
    assert bitwise(flat_state(m), flat_state(twin)) and out["policy_loss"] == float(twin.dev.losses[0].item())
    plain = make_pair(tmp_path / "c", epsilon=0.1, entropy_scale=0.0)[1]
    widen_old(plain)
    plain.train_step(s, a, R, adv)
    print("\npolicy_loss with c = 1.01: %.9g, plain %.9g" % (out["policy_loss"], float(plain.dev.losses[0].item())))
    assert not bitwise(flat_state(m)[0], flat_state(plain)[0])                        # the setting reached the step
    m.set_dual_clip(None)
    assert m.dual_clip is None and m.dev.engine_dual_clip() == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------- the buffers
import test_zzzzzzzzzzzzz_advantage_recomputation_gpu as rg  # noqa: E402  (helpers only: make(), collect(), copy_collection(), host_loop())
import test_zzzzzzzzzzzzzz_vtrace_gpu as vg  # noqa: E402  (helpers only: vt_host_loop(), BARS)
from test_zzzzzzzzzzzzz_advantage_recomputation_gpu import vae  # noqa: E402,F401  (the module-scoped MlpVAE fixture)

GAMMA, LAM = rg.GAMMA, rg.LAM
C_BUF = 1.02                                                                         # close to 1: three epochs at these sizes move the ratios a few per cent and more (tests/test_zzzzzzzzzzzzzz_vtrace_gpu.py)


def buffer_counts(buf, c):
    """The dual-clip counts of the buffer's valid rows from the tables the statistics pass read, in numpy float64, and how many rows are too close to the
    threshold c A = s for fp32 to decide the same way (within 1e-5 of |A|)."""
    valid = buf.rows.valid_rows()
    lp, lpo, A = (x.cpu().numpy()[valid].astype(np.float64) for x in (buf._logp_new, buf.logp_old, buf.advantages))
    rr = np.exp(lp - lpo)
    sur = np.minimum(rr * A, np.clip(rr, 1.0 - dc.EPS32, 1.0 + dc.EPS32) * A)
    c32 = float(np.float32(c))
    close = (A < 0) & (np.abs(c32 * A - sur) <= 1e-5 * np.abs(A))
    return dc.stats_reference(buf._logp_new.cpu().numpy(), buf.logp_old.cpu().numpy(), buf.advantages.cpu().numpy(), valid, c=c), int(close.sum()), len(valid)


@pytest.mark.parametrize("E,T,batch", rg.SHAPES)
@rg.CLASSES
def test_buffer_updates_are_their_host_loops(vae, tmp_path, continuous, E, T, batch):      # noqa: F811
    """update() with dual clip on is bitwise a host loop of the same device calls on a twin policy -- one epoch plain, and three epochs with advantage
    recomputation and V-trace on; with c = inf it is bitwise a policy that never had the setting; update_with_diagnostics reports the counts of the tables."""
    # one epoch, nothing else on
    A, m_a, _ = rg.make(vae, tmp_path / "a", continuous, E, T, False)
    B, m_b, _ = rg.make(vae, tmp_path / "b", continuous, E, T, False)
    m_a.set_dual_clip(C_BUF); m_b.set_dual_clip(C_BUF)
    rg.collect(A, 71 + E, continuous)
    rg.copy_collection(A, B)
    np.random.seed(5)
    A.update(GAMMA, LAM, num_epochs=1, batch_size=batch)
    np.random.seed(5)
    rg.host_loop(B, m_b, continuous, 1, batch)
    assert bitwise(flat_state(m_a), flat_state(m_b)) and bitwise([A.returns, A.advantages], [B.returns, B.advantages])
    # three epochs with recomputation and V-trace, against the V-trace host loop on a twin with the setting on; and with c = inf against a policy without it
    outs = {}
    for tag, c_on in (("on", C_BUF), ("inf", INF)):
        V, m_v = vg.make(vae, tmp_path / ("v" + tag), continuous, E, T)
        W, m_w = vg.make(vae, tmp_path / ("w" + tag), continuous, E, T, bars=None, recompute=False)
        m_v.set_dual_clip(c_on)
        if tag == "on":
            m_w.set_dual_clip(c_on)
        rg.collect(V, 71 + E, continuous)
        rg.copy_collection(V, W)
        np.random.seed(5)
        outs[tag] = V.update_with_diagnostics(GAMMA, LAM, num_epochs=3, batch_size=batch)
        np.random.seed(5)
        vg.vt_host_loop(W, m_w, continuous, 3, batch, vg.BARS, final_states=getattr(V, "final_states", None))
        assert bitwise(flat_state(m_v), flat_state(m_w)), tag
        assert outs[tag]["recomputed_epochs"] == 2 and len(outs[tag]["epochs"]) == 3
        want, close, n = buffer_counts(V, c_on)
        last = outs[tag]["epochs"][-1]
        print("%s %dx%d c = %s: dual_clip_fraction per epoch %s (numpy on the tables: %d of %d, %d within 1e-5 of the threshold)"
              % (type(V).__name__, E, T, c_on, [e["dual_clip_fraction"] for e in outs[tag]["epochs"]], int(want[2]), n, close))
        assert abs(round(last["dual_clip_fraction"] * n) - want[2]) <= close and last["negative_advantage_fraction"] == want[1] / n
        if close == 0:
            assert last["dual_clip_fraction"] == want[2] / n
        assert last["surrogate_mean_unclipped"] == pytest.approx(want[4] / n, rel=1e-9)
        if close == 0:
            assert last["surrogate_mean"] == pytest.approx(want[3] / n, rel=1e-9)
        assert last["surrogate_mean"] >= last["surrogate_mean_unclipped"]
    assert all(e["dual_clip_fraction"] == 0.0 and e["surrogate_mean"] == e["surrogate_mean_unclipped"] for e in outs["inf"]["epochs"])
    # switched off again: no key, no table
    Z, m_z = vg.make(vae, tmp_path / "z", continuous, E, T)
    m_z.set_dual_clip(C_BUF); m_z.set_dual_clip(None)
    rg.collect(Z, 71 + E, continuous)
    np.random.seed(5)
    out_z = Z.update_with_diagnostics(GAMMA, LAM, num_epochs=2, batch_size=batch)
    assert all("dual_clip_fraction" not in e and "surrogate_mean" not in e for e in out_z["epochs"]) and getattr(Z, "_logp_new", None) is None


def test_the_buffers_refuse_a_policy_outside_the_fused_kernels(vae, tmp_path, monkeypatch):      # noqa: F811
    import torch
    A, m, _ = rg.make(vae, tmp_path / "a", False, 3, 5, False)
    rg.collect(A, 74, False)
    m.set_dual_clip(C)
    monkeypatch.setattr(m.dev, "fused_ok", lambda: False)
    before = [x.clone() for x in (A.returns, A.advantages, m.dev.params, m.dev.params_old)]
    state = np.random.get_state()[1].copy()
    for fn in (A.update, A.update_with_diagnostics):
        with pytest.raises(ValueError, match=r"dual clip \(PPO\.set_dual_clip\) exists only in the fused kernels"):
            fn(GAMMA, LAM, num_epochs=2, batch_size=4)
    assert all(torch.equal(x, y) for x, y in zip((A.returns, A.advantages, m.dev.params, m.dev.params_old), before))
    assert np.array_equal(np.random.get_state()[1], state)
