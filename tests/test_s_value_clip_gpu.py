"""PPO2-style value-function clipping on the GPU (mi_ppo_train_step_vclip, mi_ppo_value_clip_stats, PPO.set_value_clip and the rollout buffers).

Engines: 2 actions on the reference trunk (67 -> 500 / 300: the <2> instantiation of the head / loss kernel) and 3 actions on the small trunk of
tests/ppo_shape_cases.py's B5 cases (5 -> 36 / 20: the <8> instantiation); minibatches of M = 5 (one partial block of the loss kernel), 33 (a second block that
holds one sample) and 257 (the chunked weight-gradient route), each as contiguous tensors and through row_idx into tables of 2 M + 3 rows whose old_values are NaN in
every row the index does not name; fp32 and bf16x3.

The inputs are planned on the reference alone: V in float64 with numpy from export_params(), eps_v = 0.2, and sample i is put into class i mod 5 by its V_old and R
  0  inside the range: |V - V_old| = 0.05 (both signs), R = V +- 0.7                      l_c == l_u, the plain gradient
  1  V above the range (V_old = V - 0.6), R = V - 1.0 on V_old's side                      l_u = 1.00 > l_c = 0.36: the gradient flows
  2  V above the range (V_old = V - 0.6), R = V + 0.5 beyond V                             l_c = 0.81 > l_u = 0.25: the gradient is zero
  3, 4  the mirror images below the range
so V is 0.4 from the range's edge and the two terms are 0.56 or more apart: far above any fp32 or bf16x3 value error (~1e-5 of the value's scale), no sample is left
out.  plan() asserts the classes and margins on the float64 values of the fp32 inputs.  The float64 reference is oracle.ppo_oracle.ppo_losses with its value term
replaced by the definition of include/mi355_carla.h; bounds are the project's (tests/ppo_shape_cases.py, tests/test_j_ppo_bf16x3_gpu.py,
tests/test_p_rollout_diagnostics_gpu.py)."""
import ctypes
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ppo_shape_cases as pc  # noqa: E402
from oracle import ppo_oracle as po  # noqa: E402
from rollout_gpu_common import bitwise, flat_state, inputs, make_pair, make_world  # noqa: E402

EPS_V = 0.2
EPS32 = float(np.float32(EPS_V))                          # the range as the kernels see it
INF = float("inf")
ALPHA = 1e-4
MS = (5, 33, 257)
# name -> (input_dim, num_actions, hidden, seed, perturb): the reference trunk with its 2 actions, and ppo_shape_cases' B5 shape with 3
SHAPES = OrderedDict([("A2", (67, 2, (500, 300), 2, 0.02)), ("A3", (5, 3, (36, 20), 11, 0.0231))])
VALUE_NET = ("policy/dense_2/kernel", "policy/dense_2/bias", "policy/dense_3/kernel", "policy/dense_3/bias", "policy/value/kernel", "policy/value/bias")
POLICY_NET = ("policy/dense/kernel", "policy/dense/bias", "policy/dense_1/kernel", "policy/dense_1/bias", "policy/action_mean/kernel", "policy/action_mean/bias",
              "policy/action_logstd")
X3_GRAD_FLOOR, X3_GRAD_FACTOR = 1e-3, 4.0                # tests/test_j_ppo_bf16x3_gpu.py: max(1e-3, 4 x the fp32 oracle's own distance from float64)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def value64(p, s):
    """The value net in float64 with numpy on exported (fp32) parameters."""
    f = lambda k: np.asarray(p[k], np.float64)      # noqa: E731
    g = np.maximum(s.astype(np.float64) @ f("policy/dense_2/kernel") + f("policy/dense_2/bias"), 0.0)
    g = np.maximum(g @ f("policy/dense_3/kernel") + f("policy/dense_3/bias"), 0.0)
    return (g @ f("policy/value/kernel") + f("policy/value/bias")).reshape(-1)


def plan(V):
    """float64 V [M] -> (V_old fp32, R fp32, class [M]); asserts the classes and margins on the float64 values of what it returns."""
    M = len(V)
    k = np.arange(M) % 5
    sgn = np.where((np.arange(M) // 5) % 2 == 0, 1.0, -1.0)
    v_old = np.select([k == 0, (k == 1) | (k == 2)], [V + 0.05 * sgn, V - (EPS_V + 0.4)], V + (EPS_V + 0.4)).astype(np.float32)
    R = np.select([k == 0, k == 1, k == 2, k == 3], [V + 0.7 * sgn, V - 1.0, V + 0.5, V + 1.0], V - 0.5).astype(np.float32)
    vo, r = v_old.astype(np.float64), R.astype(np.float64)
    d = V - vo
    vc = np.minimum(np.maximum(V, vo - EPS32), vo + EPS32)
    lu, lc = (V - r) ** 2, (vc - r) ** 2
    inside = k == 0
    assert np.all(np.abs(np.abs(d[inside]) - 0.05) < 1e-5) and np.all(lc[inside] == lu[inside])
    assert np.all(np.abs(d[~inside]) - EPS32 >= 0.39)                                # 0.4 from the range's edge
    assert np.all(d[(k == 1) | (k == 2)] > 0) and np.all(d[(k == 3) | (k == 4)] < 0)
    flows, zero = (k == 1) | (k == 3), (k == 2) | (k == 4)
    assert np.all(lu[flows] - lc[flows] >= 0.5) and np.all(lc[zero] - lu[zero] >= 0.5)
    return v_old, R, k


def reference(c, v_old, R, dtype):
    """oracle.ppo_oracle.ppo_losses in `dtype` with the value term of the definition: value_loss = value_scale * mean(max(l_u, l_c)), the gradient of a sample
    going to l_u unless l_c > l_u (where the clamp's slope is 0) -> (scalars, 13 gradients, l_c > l_u per sample)."""
    import torch
    t = lambda x: torch.from_numpy(np.asarray(x, np.float32)).to(dtype)      # noqa: E731
    p = OrderedDict((k, t(v).requires_grad_(True)) for k, v in c.theta.items())
    L = po.ppo_losses(p, {k: t(v) for k, v in pc.old_names(c.theta_old).items()}, t(c.s), t(c.a), t(R), t(c.adv), c.low, c.high, pc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE)
    v, vo, eps = L["value"], t(v_old), torch.tensor(EPS32, dtype=dtype)
    vc = torch.minimum(torch.maximum(v, vo - eps), vo + eps)
    lu, lc = (v - t(R)) ** 2, (vc - t(R)) ** 2
    zero = (lc > lu).detach()
    value_loss = torch.where(zero, lc.detach(), lu).mean() * pc.VALUE_SCALE
    loss = -L["policy_loss"] + value_loss - L["entropy_loss"]
    loss.backward()
    grads = OrderedDict((k, (x.grad if x.grad is not None else torch.zeros_like(x)).numpy()) for k, x in p.items())
    return dict(value_loss=float(value_loss.detach()), loss=float(loss.detach())), grads, zero.numpy()


class Problem:
    pass


class Rig:
    """One engine per (shape, precision) and its problems per M: contiguous tensors, the same samples as shuffled rows of tables, the cached log pi_old."""

    def __init__(self, shape, precision):
        import torch
        from mi355.ppo_device import PpoDevice
        self.shape, self.precision = shape, precision
        self.din, self.A, self.hidden, self.seed, self.perturb = SHAPES[shape]
        low, high = pc.bounds(self.A)
        self.d = PpoDevice(self.din, self.A, low, high, pc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE, hidden=self.hidden, max_batch=320, precision=precision)
        assert self.d.fused_ok()
        self.used = torch.zeros(self.d.n_flat, dtype=torch.bool, device=self.d.device)
        for _, (o_, s_) in self.d.layout.items():
            self.used[o_:o_ + s_] = True
        self.problems = {}

    def restore(self, q, fill=4.25):
        """The problem's parameters (every M has its own: ppo_shape_cases.build draws them with the samples), zero optimiser state, a marked gradient buffer."""
        d = self.d
        for x, y in zip((d.params, d.adam_m, d.adam_v, d.params_old), q.state0 + [q.old]):
            x.copy_(y)
        d.grads.fill_(fill)
        d.set_max_grad_norm(None)

    def up(self, x):
        import torch
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.d.device)

    def problem(self, M):
        import torch
        if M in self.problems:
            self.restore(self.problems[M])
            return self.problems[M]
        d = self.d
        q = Problem()
        q.M = M
        q.c = c = pc.build(self.din, self.A, self.hidden, M, self.seed, self.perturb, reference=False)
        d.load_params(c.theta, pc.old_names(c.theta_old))
        d.adam_m.zero_(); d.adam_v.zero_()
        q.state0, q.old = [x.clone() for x in (d.params, d.adam_m, d.adam_v)], d.params_old.clone()
        exported = d.export_params()
        assert all(np.array_equal(exported[k], c.theta[k]) for k in c.theta)
        q.V = value64(exported, c.s)
        q.v_old, q.R, q.cls = plan(q.V)
        q.v_same = q.V.astype(np.float32)                                            # V_old = the float64 V rounded to fp32: nothing is clipped at eps_v = 0.2
        q.s, q.a, q.adv, q.Rd = self.up(c.s), self.up(c.a), self.up(c.adv), self.up(q.R)
        q.vo, q.vs = self.up(q.v_old), self.up(q.v_same)
        q.lp = torch.empty(M, device=d.device)
        d.logp_old(q.s, q.a, M, q.lp)
        # the same samples as rows of tables of 2 M + 3 rows: the other rows hold other finite samples, and NaN where old values would be
        n = 2 * M + 3
        rng = np.random.RandomState(100 + M)
        rows = rng.permutation(n)[:M].astype(np.int32)
        q.rows = torch.from_numpy(rows).to(d.device)
        idx = q.rows.long()
        q.tab = {}
        for name, x, width in (("s", q.s, self.din), ("a", q.a, self.A), ("R", q.Rd, 0), ("adv", q.adv, 0), ("lp", q.lp, 0)):
            t = self.up(0.5 * rng.standard_normal((n, width) if width else (n,)))
            t[idx] = x
            q.tab[name] = t
        for name, x in (("vo", q.vo), ("vs", q.vs)):
            t = torch.full((n,), float("nan"), device=d.device)
            t[idx] = x
            q.tab[name] = t
        self.problems[M] = q
        return q

    def step(self, q, form, v_old=None, eps=None, adam=True, comm=None, cached=True):
        """One step from state0 -> (params / m / v, losses, gradient buffer, dv).  v_old None: the EXISTING entry of this form (adam False: forward_backward, which has no
        cache); else mi_ppo_train_step_vclip with v_old "vo" (the planned values) or "vs" (V itself)."""
        d, M = self.d, q.M
        a = (1.0 / M, 1.0, ALPHA)
        tabs = (q.tab["s"], q.tab["a"], q.tab["R"], q.tab["adv"])
        flat = (q.s, q.a, q.Rd, q.adv)
        lp_f, lp_t = (q.lp, q.tab["lp"]) if cached else (None, None)
        if v_old is None:
            if not adam:
                assert form == "flat" and not cached
                d.forward_backward(*flat, M, 1.0 / M, 1.0)
            elif comm is not None:
                d.train_step_dp(comm, *(flat if form == "flat" else tabs), lp_f if form == "flat" else lp_t, None if form == "flat" else q.rows, M, *a)
            elif form == "flat":
                d.train_step(*flat, M, *a, logp_old=lp_f)
            else:
                d.train_step_idx(*tabs, lp_t, q.rows, M, *a)
        elif form == "flat":
            d.train_step_vclip(comm, *flat, lp_f, getattr(q, v_old), eps, None, M, *a, adam=adam)
        else:
            d.train_step_vclip(comm, *tabs, lp_t, q.tab[v_old], eps, q.rows, M, *a, adam=adam)
        return [x.clone() for x in (d.params, d.adam_m, d.adam_v)], d.losses.clone(), d.grads.clone(), d.value_head_grad[:M].clone()


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(shape, precision):
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


GRID = [(s, p, M) for s in SHAPES for p in ("fp32", "bf16x3") for M in MS]


@pytest.mark.parametrize("shape,precision,M", GRID)
def test_nothing_clipped_is_the_existing_step_bit_for_bit(rigs, recording_comm, shape, precision, M):
    """eps_v = inf on the planned (mixed) old values, and eps_v = 0.2 with V_old = V: parameters, optimiser state and losses of mi_ppo_train_step / _idx / _dp (on a
    recording communicator) with the cached log pi_old, and the gradient buffer of mi_ppo_forward_backward (adam = 0, the old policy's forward inside the step)."""
    r = rigs(shape, precision)
    q = r.problem(M)
    for form, comm in (("flat", None), ("idx", None), ("flat", recording_comm), ("idx", recording_comm)):
        r.restore(q)
        want = r.step(q, form, comm=comm)
        for v_old, eps in (("vo", INF), ("vs", EPS_V)):
            r.restore(q)
            got = r.step(q, form, v_old, eps, comm=comm)
            tag = (shape, precision, M, form, comm is not None, v_old, eps)
            assert bitwise(got[0], want[0]) and bitwise(got[1], want[1]) and bitwise(got[2], want[2]), tag
    r.restore(q)
    want = r.step(q, "flat", adam=False, cached=False)
    assert bool((want[2][r.used] != 4.25).any())
    for v_old, eps in (("vo", INF), ("vs", EPS_V)):
        r.restore(q)
        got = r.step(q, "flat", v_old, eps, adam=False, cached=False)
        assert bitwise(got[2], want[2]) and bitwise(got[1], want[1]) and bitwise(got[0], want[0]), (shape, precision, M, v_old, eps)
    r.restore(q)


_REF = {}


def float64_reference(r, q):
    key = (r.shape, q.M)
    if key not in _REF:
        import torch
        c = q.c
        scal, g64, zero = reference(c, q.v_old, q.R, torch.float64)
        _, g32, _ = reference(c, q.v_old, q.R, torch.float32)
        assert np.array_equal(zero, (q.cls == 2) | (q.cls == 4))
        _REF[key] = (scal, g64, {k: rel_err(g32[k], g64[k]) for k in g64})
    return _REF[key]


@pytest.mark.parametrize("form", ["flat", "idx"])
@pytest.mark.parametrize("shape,precision,M", GRID)
def test_mixed_classes_against_float64(rigs, shape, precision, M, form):
    r = rigs(shape, precision)
    q = r.problem(M)
    scal, g64, d32 = float64_reference(r, q)
    r.restore(q)
    params, losses, _, dv = r.step(q, form, "vo", EPS_V, adam=False)
    g = r.d.export_grads()
    L = losses.cpu().numpy().astype(np.float64)
    print("\n%s %s M = %d %s: value_loss %.9g (float64 %.9g, rel %.2e), loss rel %.2e" %
          (shape, precision, M, form, L[1], scal["value_loss"], abs(L[1] - scal["value_loss"]) / scal["value_loss"], abs(L[3] - scal["loss"]) / abs(scal["loss"])))
    assert L[1] == pytest.approx(scal["value_loss"], rel=1e-4) and L[3] == pytest.approx(scal["loss"], rel=1e-4)
    bound = {k: pc.GRAD_REL if precision == "fp32" else max(X3_GRAD_FLOOR, X3_GRAD_FACTOR * d32[k]) for k in VALUE_NET}
    err = {k: rel_err(g[k], g64[k]) for k in VALUE_NET}
    for k in VALUE_NET:
        print("  %-26s %.3e of max (bound %.1e)" % (k, err[k], bound[k]))
    assert not {k: (err[k], bound[k]) for k in VALUE_NET if err[k] > bound[k]}
    # the value head's own gradient per sample: exactly zero in the two zero-gradient classes, flowing everywhere else
    dv = dv.cpu().numpy()
    zero = (q.cls == 2) | (q.cls == 4)
    assert np.all(dv[zero] == 0.0) and np.all(dv[~zero] != 0.0), dv
    # (a flowing gradient is 2 value_scale (V - R) / M with |V - R| >= 0.5: the project's bound on a predicted value, rtol 1e-4 / atol 1e-5, times 2 / M)
    want_dv = np.where(zero, 0.0, 2.0 * pc.VALUE_SCALE * (q.V - q.R.astype(np.float64)) / M)
    # (bf16x3: the split products drop ~2^-16 = 1.5e-5 of each term, through three layers of O(1) activations: 1e-4 absolute on V, the mode's loss tolerance)
    v_tol = pc.ACT_RTOL * np.abs(q.V) + pc.ACT_ATOL if precision == "fp32" else 1e-4
    assert np.all(np.abs(dv - want_dv) <= 1e-6 * np.abs(want_dv) + (2.0 * pc.VALUE_SCALE / M) * v_tol), np.abs(dv - want_dv).max()
    # nothing on the policy side changes: bitwise the unclipped step's (eps_v = inf, which the test above ties to the existing entries)
    r.restore(q)
    _, losses_u, _, dv_u = r.step(q, form, "vo", INF, adam=False)
    g_u = r.d.export_grads()
    for k in POLICY_NET:
        assert np.array_equal(g[k].view(np.int32), g_u[k].view(np.int32)), k
    Lu = losses_u.cpu().numpy()
    Lc = losses.cpu().numpy()
    assert all(Lc[i].tobytes() == Lu[i].tobytes() for i in (0, 2, 4)) and np.array_equal(Lc[5:].view(np.int32), Lu[5:].view(np.int32))
    # the value side does change.  (Not the value bias: its gradient is the sum of dv, and the two zero-gradient classes are planned with V - R = -0.5 and +0.5, so
    # what they would have added cancels -- exactly so at M = 5.  The head kernel's gradient weighs every sample with its own h2 row.)
    dv_u = dv_u.cpu().numpy()
    assert np.all(dv_u != 0.0) and np.array_equal(dv_u[~zero].view(np.int32), dv[~zero].view(np.int32)) and Lc[1] > Lu[1]
    assert not np.array_equal(g["policy/value/kernel"], g_u["policy/value/kernel"])
    assert bitwise(params, q.state0)                                                 # adam = 0 leaves the parameters and the optimiser state alone
    r.restore(q)


@pytest.mark.parametrize("form", ["flat", "idx"])
@pytest.mark.parametrize("shape,precision,M", GRID)
def test_reproducible_and_the_global_norm_route(rigs, shape, precision, M, form):
    import torch
    r = rigs(shape, precision)
    q, d = r.problem(M), r.d
    r.restore(q)
    first = r.step(q, form, "vo", EPS_V)
    r.restore(q)
    again = r.step(q, form, "vo", EPS_V)
    assert all(bitwise(x, y) for x, y in zip(first, again))
    assert not bitwise(first[0][0], q.state0[0])
    # with clipping by the global norm: twice the same, and "gradient buffer x factor, then mi_ppo_apply_adam" bit for bit
    runs = []
    for _ in range(2):
        r.restore(q)
        d.set_max_grad_norm(0.5)
        runs.append(r.step(q, form, "vo", EPS_V) + (d.grad_clip.clone(),))
    assert all(bitwise(x, y) for x, y in zip(runs[0], runs[1]))
    rec = runs[0][4]
    assert rec[2].item() == 0.5 and 0.0 < rec[1].item() <= 1.0 and rec[0].item() > 0.0
    r.restore(q)
    r.step(q, form, "vo", EPS_V, adam=False)
    d.grads.mul_(rec[1])
    d.apply_adam(ALPHA)
    assert bitwise([d.params, d.adam_m, d.adam_v], runs[0][0]), (shape, precision, M, form, rec)
    assert not bool(runs[0][2].any()) and torch.equal(runs[0][1], first[1])       # the gradient buffer is zero afterwards; the losses do not depend on the route
    r.restore(q)


def stats_reference(v, vo, R, rows):
    v, vo, R = (x[rows].astype(np.float64) for x in (v, vo, R))
    vc = np.minimum(np.maximum(v, vo - EPS32), vo + EPS32)
    lu, lc = (v - R) ** 2, (vc - R) ** 2
    return np.array([len(rows), (np.abs(v - vo) > EPS32).sum(), np.maximum(lu, lc).sum(), (lc > lu).sum()], np.float64)


@pytest.mark.parametrize("shape,M", [(s, M) for s in SHAPES for M in MS])
def test_value_clip_stats(rigs, shape, M):
    import torch
    from mi355.ppo_device import N_STATS, N_VCLIP_STATS, value_clip_summary
    r = rigs(shape, "fp32")
    q, d = r.problem(M), r.d
    r.restore(q)
    n = q.tab["R"].shape[0]
    f64 = lambda k: torch.zeros(k, dtype=torch.float64, device=d.device)      # noqa: E731
    v_new = torch.full((n,), float("nan"), device=d.device)                          # V under the current parameters, by the statistics pass, at the named rows only
    d.update_stats(q.tab["s"], q.tab["a"], q.tab["R"], q.tab["lp"], q.rows, M, f64(N_STATS), f64(d.stats_scratch_doubles(M)), value_out=v_new)
    rows = q.rows.cpu().numpy()
    named = np.zeros(n, bool)
    named[rows] = True
    v_host = v_new.cpu().numpy()
    assert np.all(np.isnan(v_host[~named])) and np.allclose(v_host[rows], q.V, rtol=1e-4, atol=1e-5)
    assert np.all(np.isnan(q.tab["vo"].cpu().numpy()[~named]))
    assert d.value_clip_scratch_doubles(M) == N_VCLIP_STATS * ((M + 255) // 256)

    def run(v, vo, R, idx, m, stats, accumulate=False):
        scratch = torch.full((d.value_clip_scratch_doubles(m),), -1.0, dtype=torch.float64, device=d.device)
        d.value_clip_stats(v, vo, R, idx, m, EPS_V, stats, scratch, accumulate=accumulate)
        return stats.cpu().numpy()
    got = run(v_new, q.tab["vo"], q.tab["R"], q.rows, M, torch.full((N_VCLIP_STATS,), 7.0, dtype=torch.float64, device=d.device)).copy()
    want = stats_reference(v_host, q.tab["vo"].cpu().numpy(), q.tab["R"].cpu().numpy(), rows)
    print("\n%s M = %d: sums %s, numpy float64 %s" % (shape, M, got, want))
    assert got[0] == M and got[1] == (q.cls != 0).sum() and got[3] == ((q.cls == 2) | (q.cls == 4)).sum()       # exact against the planned classes
    assert got[0] == want[0] and got[1] == want[1] and got[3] == want[3]
    assert abs(got[2] - want[2]) <= 1e-9 * want[2]
    assert run(v_new, q.tab["vo"], q.tab["R"], q.rows, M, f64(N_VCLIP_STATS)).tobytes() == got.tobytes()        # run to run
    # NaN in the rows that are not named changes nothing: the same samples gathered into tables of exactly M rows
    idx = q.rows.long()
    dense = run(v_new[idx].contiguous(), q.vo, q.Rd, torch.arange(M, dtype=torch.int32, device=d.device), M, f64(N_VCLIP_STATS))
    assert dense.tobytes() == got.tobytes()
    # two chunks with accumulate: counts bitwise, the sum within 1e-12
    cut = max(1, M // 3)
    acc = f64(N_VCLIP_STATS)
    run(v_new, q.tab["vo"], q.tab["R"], q.rows[:cut].contiguous(), cut, acc)
    chunked = run(v_new, q.tab["vo"], q.tab["R"], q.rows[cut:].contiguous(), M - cut, acc, accumulate=True)
    assert chunked[[0, 1, 3]].tobytes() == got[[0, 1, 3]].tobytes() and abs(chunked[2] - got[2]) <= 1e-12 * got[2]
    s = value_clip_summary(got)
    assert s["value_clip_fraction"] == (q.cls != 0).mean() and s["value_grad_zero_fraction"] == ((q.cls == 2) | (q.cls == 4)).mean()
    assert s["value_loss_clipped"] == got[2] / M
    # nothing but scratch and stats is written
    assert bitwise([d.params, d.adam_m, d.adam_v], q.state0)


def test_engine_side_argument_errors(rigs):
    from mi355 import lib as milib
    r = rigs("A3", "fp32")
    q, d = r.problem(5), r.d
    with pytest.raises(milib.MiError, match=r"mi_ppo_train_step_vclip failed \(-1\): mi_ppo_train_step_vclip: batch outside"):
        d.L.mi_ppo_train_step_vclip(d.handle, None, d.stream(), q.s.data_ptr(), q.a.data_ptr(), q.Rd.data_ptr(), q.adv.data_ptr(), None, q.vo.data_ptr(), EPS_V, None, 0,
                                    d.max_batch + 1, 0.2, 1.0, 1, ALPHA, 0.9, 0.999, 1e-8)
    for bad in (0.0, -0.2, float("nan")):
        with pytest.raises(milib.MiError, match="clip_range_vf"):
            d.train_step_vclip(None, q.s, q.a, q.Rd, q.adv, None, q.vo, bad, None, 5, 0.2, 1.0, ALPHA)
    with pytest.raises(milib.MiError, match="missing old_values"):
        d.train_step_vclip(None, q.s, q.a, q.Rd, q.adv, None, None, EPS_V, None, 5, 0.2, 1.0, ALPHA)
    assert bitwise([d.params, d.adam_m, d.adam_v], q.state0)


def test_no_per_layer_form(tmp_path):
    """An engine outside the fused kernels' range (padded input width 104 > 96) refuses the clipped step with MI_ERR_SHAPE instead of running an unclipped one."""
    import torch
    from mi355 import lib as milib
    from mi355.ppo_device import PpoDevice
    low, high = pc.bounds(3)
    d = PpoDevice(100, 3, low, high, pc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE, hidden=(64, 64), max_batch=32)
    assert not d.fused_ok()
    z = lambda *s: torch.zeros(*s, device=d.device)      # noqa: E731
    before = d.params.clone()
    with pytest.raises(milib.MiError, match=r"mi_ppo_train_step_vclip failed \(-2\).*no per-layer form"):
        d.train_step_vclip(None, z(5, 100), z(5, 3), z(5), z(5), None, z(5), EPS_V, None, 5, 0.2, 1.0, ALPHA)
    assert torch.equal(d.params, before)
    d.close()


# ---- end to end: rollout buffers of 4 environments x 8 steps, scripted frames ----
E, T, BATCH, EPOCHS, SEED = 4, 8, 8, 2, 3
VCLIP_KEYS = {"value_clip_fraction", "value_loss_clipped", "value_grad_zero_fraction"}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return make_world(tmp_path_factory, "value_clip", policy=False)


def collect(world, tmp, continuous, source):
    """A policy and a full E x T collection through the buffer's own step; the device tables are those of the first collection (the recording step's split-K layers
    end in fp32 atomics, so two collections of the same frames can differ in the last bit).  continuous: lane 1 reports a done at its step 3."""
    from rollout import ContinuousRolloutBuffer, RolloutBuffer
    _, m = make_pair(tmp)
    buf = (ContinuousRolloutBuffer if continuous else RolloutBuffer)(world["vae"], m, E, T)
    rng = np.random.RandomState(571)
    buf.reset()
    for t in range(1, T + 1):
        f, ms, nz = inputs(rng, E)
        buf.step(f, ms, noise=nz)
        buf.outcome(rng.uniform(0, 1, E), np.array([continuous and e == 1 and t == 3 for e in range(E)]))
    f, ms, _ = inputs(rng, E)
    if continuous:
        need = buf.rows.needs_bootstrap()
        buf.bootstrap(f[need], ms[need], env_ids=need)
    else:
        buf.bootstrap(f, ms)
    mine = [buf.states, buf.actions, buf.values]
    if not source:
        source.extend(x.clone() for x in mine)
    for x, y in zip(mine, source):
        x.copy_(y)
    np.random.seed(SEED)
    return m, buf


@pytest.mark.parametrize("continuous", [False, True])
def test_rollout_buffer_update_end_to_end(world, tmp_path, continuous):
    import torch
    from ppo import ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON, _adam_alpha
    source = []
    # the parent's behaviour: a policy whose setter is never called
    m0, b0 = collect(world, tmp_path / "w0", continuous, source)
    assert m0.value_clip is None
    out0 = b0.update_with_diagnostics(num_epochs=EPOCHS, batch_size=BATCH)
    # value clipping on
    m1, b1 = collect(world, tmp_path / "w1", continuous, source)
    m1.set_value_clip(EPS_V)
    values_before = b1.values.clone()
    out1 = b1.update(num_epochs=EPOCHS, batch_size=BATCH)
    assert set(out1) == set(out0) - {"epochs", "epochs_run", "stopped_early"}
    assert torch.equal(b1.values, values_before)                                     # the recorded values are read, never written
    # (at a learning rate of 1e-4 no value moves 0.2 in 8 steps: this update exercises the route, the update with a tiny range below exercises the clipping)
    # a host loop of PpoDevice.train_step_vclip over the same permutations, from the tables the update left (returns, advantages, log pi_old under theta_old)
    _, m2 = make_pair(tmp_path / "w2")
    m2.update_old_policy()
    valid = b1.rows.valid_rows()
    np.random.seed(SEED)
    b1p, b2p = np.float32(ADAM_BETA1), np.float32(ADAM_BETA2)
    records = []
    for _ in range(EPOCHS):
        indices = np.arange(len(valid))
        np.random.shuffle(indices)
        perm = torch.from_numpy(valid[indices]).to(b1.device)
        for i in range(0, len(valid), BATCH):
            mb = perm[i:i + BATCH]
            k = int(mb.numel())
            m2.dev.train_step_vclip(None, b1.states, b1.actions, b1.returns, b1.advantages, b1.logp_old, b1.values, EPS_V, mb, k, 1.0 / k, 1.0,
                                    _adam_alpha(m2.current_learning_rate(), b1p, b2p), ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON)
            records.append(m2.dev.losses.clone())
            b1p, b2p = np.float32(b1p * np.float32(ADAM_BETA1)), np.float32(b2p * np.float32(ADAM_BETA2))
    assert bitwise(flat_state(m2), flat_state(m1))
    assert np.array_equal(torch.stack(records).cpu().numpy()[:, 1].astype(np.float64), [rec["value_loss"] for rec in out1["losses"]])
    # update_with_diagnostics: the same parameters, and the three keys in every epoch
    m3, b3 = collect(world, tmp_path / "w3", continuous, source)
    m3.set_value_clip(EPS_V)
    out3 = b3.update_with_diagnostics(num_epochs=EPOCHS, batch_size=BATCH)
    assert bitwise(flat_state(m3), flat_state(m1))
    assert set(out3) == set(out0) and len(out3["epochs"]) == EPOCHS
    for rec, rec0 in zip(out3["epochs"], out0["epochs"]):
        assert set(rec) == set(rec0) | VCLIP_KEYS
        assert 0.0 <= rec["value_grad_zero_fraction"] <= rec["value_clip_fraction"] <= 1.0
        assert rec["value_loss_clipped"] >= rec["value_mse"] * (1 - 1e-12)           # max(l_u, l_c) >= l_u per sample, both in double from the same fp32 values
        if rec["value_clip_fraction"] == 0.0:
            assert rec["value_loss_clipped"] == pytest.approx(rec["value_mse"], rel=1e-12)
    # the last epoch's figures against numpy on the tables: V under the final parameters is what the statistics pass left in its table
    v_new, vo, R = b3._values_new.cpu().numpy(), b3.values.cpu().numpy(), b3.returns.cpu().numpy()
    want = stats_reference(v_new, vo, R, valid)
    last = out3["epochs"][-1]
    assert last["value_clip_fraction"] == want[1] / want[0] and last["value_grad_zero_fraction"] == want[3] / want[0]
    assert last["value_loss_clipped"] == pytest.approx(want[2] / want[0], rel=1e-9)
    # a range the values leave within a step or two: samples are clipped, and the parameters are no longer the unclipped twin's
    m5, b5 = collect(world, tmp_path / "w5", continuous, source)
    m5.set_value_clip(1e-5)
    out5 = b5.update_with_diagnostics(num_epochs=EPOCHS, batch_size=BATCH)
    assert out5["epochs"][-1]["value_clip_fraction"] > 0.0 and out5["epochs"][-1]["value_grad_zero_fraction"] > 0.0
    assert not bitwise(flat_state(m5), flat_state(m0))
    # switched on and off again: the parent's keys and parameters
    m4, b4 = collect(world, tmp_path / "w4", continuous, source)
    m4.set_value_clip(EPS_V)
    m4.set_value_clip(None)
    out4 = b4.update_with_diagnostics(num_epochs=EPOCHS, batch_size=BATCH)
    assert set(out4) == set(out0) and all(set(x) == set(y) for x, y in zip(out4["epochs"], out0["epochs"]))
    assert bitwise(flat_state(m4), flat_state(m0)) and getattr(b4, "_values_new", None) is None
    assert out4["epochs"] == out0["epochs"] and out4["losses"] == out0["losses"]
    # PPO.train refuses to run an unclipped step while the setting is on
    with pytest.raises(ValueError, match="value clipping is on"):
        m3.train(np.zeros((4, 67), np.float32), np.zeros((4, 2), np.float32), np.zeros(4, np.float32), np.zeros(4, np.float32))


def test_a_policy_outside_the_fused_kernels_is_refused_before_any_launch(world, tmp_path, monkeypatch):
    """More than 8 actions get no engine at all (mi_ppo_create's descriptor check), so the buffers' up-front check is reached through what it asks:
    PpoDevice.fused_ok().  The refusal comes before the finish call: tables, parameters and the numpy stream are what they were."""
    import torch
    from mi355 import lib as milib
    from ppo import PPO

    class Nine:
        shape = (9,)
        low, high = -np.ones(9, np.float32), np.ones(9, np.float32)
    m9 = PPO(np.array([67]), Nine(), model_dir=str(tmp_path / "nine"), seed=2)
    m9.set_value_clip(EPS_V)
    with pytest.raises(milib.MiError):
        m9.init_session(init_logging=False)
    m, buf = collect(world, tmp_path / "w", False, [])
    m.set_value_clip(EPS_V)
    monkeypatch.setattr(m.dev, "fused_ok", lambda: False)
    before = [x.clone() for x in (buf.returns, buf.advantages, buf.logp_old, m.dev.params, m.dev.params_old)]
    state = np.random.get_state()[1].copy()
    for fn in (buf.update, buf.update_with_diagnostics):
        with pytest.raises(ValueError, match="value clipping"):
            fn(num_epochs=EPOCHS, batch_size=BATCH)
    assert all(torch.equal(x, y) for x, y in zip((buf.returns, buf.advantages, buf.logp_old, m.dev.params, m.dev.params_old), before))
    assert np.array_equal(np.random.get_state()[1], state)
