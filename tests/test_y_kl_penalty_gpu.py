"""The adaptive KL penalty on the GPU: mi_ppo_old_policy_cache, mi_ppo_train_step_kl, mi_ppo_kl_stats_idx, PPO.set_kl_penalty and the rollout buffers.

Engines, sizes, inputs, the float64 reference and the bound on the KL scalar: tests/kl_penalty_cases.py.  Each size runs as contiguous tensors and through row_idx into
tables of 2 M + 3 rows whose mean_old / logp_old (and old values) are NaN in every row the index does not name; fp32 and bf16x3.  Bounds are the project's: loss
scalars 1e-4 relative, gradients 2e-4 of each tensor's max (bf16x3: max(1e-3, 4 x the fp32 oracle's own distance from float64)), means rtol 1e-4 / atol 1e-5.
No sample is left out of any comparison."""
import ctypes
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kl_penalty_cases as kc  # noqa: E402
import ppo_shape_cases as pc  # noqa: E402
from rollout_gpu_common import bitwise, flat_state, inputs, make_pair, make_world  # noqa: E402

ALPHA = 1e-4
EPS_V = 0.2
SENT = -777.0
X3_GRAD_FLOOR, X3_GRAD_FACTOR = 1e-3, 4.0                # tests/test_j_ppo_bf16x3_gpu.py
GRID = [(s, p, M) for s in kc.SHAPES for p in ("fp32", "bf16x3") for M in kc.MS]


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


class Problem:
    pass


class Rig:
    """One engine per (shape, precision) and its problems per M: contiguous tensors, the same samples as shuffled rows of tables, the old policy's cache."""

    def __init__(self, shape, precision):
        import torch
        from mi355.ppo_device import PpoDevice
        self.shape, self.precision = shape, precision
        self.din, self.A, self.hidden, _, _ = kc.SHAPES[shape]
        low, high = pc.bounds(self.A)
        self.d = PpoDevice(self.din, self.A, low, high, pc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE, hidden=self.hidden, max_batch=320, precision=precision)
        assert self.d.fused_ok()
        self.used = torch.zeros(self.d.n_flat, dtype=torch.bool, device=self.d.device)
        for _, (o_, s_) in self.d.layout.items():
            self.used[o_:o_ + s_] = True
        self.problems = {}

    def restore(self, q, fill=4.25):
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
        d, A = self.d, self.A
        q = Problem()
        q.M = M
        q.c, q.ref = kc.case(self.shape, M)
        c = q.c
        d.load_params(c.theta, pc.old_names(c.theta_old))
        d.adam_m.zero_(); d.adam_v.zero_()
        q.state0, q.old = [x.clone() for x in (d.params, d.adam_m, d.adam_v)], d.params_old.clone()
        q.s, q.a, q.adv, q.Rd = self.up(c.s), self.up(c.a), self.up(c.adv), self.up(c.R)
        # the old policy's cache, eight sentinels behind each output
        q.lp_buf, q.mo_buf = torch.full((M + 8,), SENT, device=d.device), torch.full((M * A + 8,), SENT, device=d.device)
        q.lp, q.mo = q.lp_buf[:M], q.mo_buf[:M * A].view(M, A)
        d.old_policy_cache(q.s, q.a, M, q.lp, q.mo)
        q.mo_host = q.mo.cpu().numpy().copy()
        rng = np.random.RandomState(300 + M)
        # old values of the combination with value clipping, planned on the float64 V: even samples have V 0.5 outside the range on the far side of R (the clipped
        # term is the larger one by >= 0.09 + 0.6 |V - R|: no value gradient), odd samples V_old = V (nothing clipped)
        V = q.ref["value"]
        q.vo = self.up(np.where(np.arange(M) % 2 == 0, V + 0.5 * np.where(V >= c.R, 1.0, -1.0), V))
        n = 2 * M + 3
        rows = rng.permutation(n)[:M].astype(np.int32)
        q.rows = torch.from_numpy(rows).to(d.device)
        idx = q.rows.long()
        q.tab = {}
        for name, x, width in (("s", q.s, self.din), ("a", q.a, A), ("R", q.Rd, 0), ("adv", q.adv, 0)):
            t = self.up(0.5 * rng.standard_normal((n, width) if width else (n,)))
            t[idx] = x
            q.tab[name] = t
        for name, x, width in (("lp", q.lp, 0), ("mo", q.mo, A), ("vo", q.vo, 0)):
            t = torch.full((n, width) if width else (n,), float("nan"), device=d.device)
            t[idx] = x
            q.tab[name] = t
        self.problems[M] = q
        self.restore(q)
        return q

    def step(self, q, form, beta=None, cached=True, adam=True, comm=None, vclip=False):
        """One step from the state the engine is in -> (params / m / v, losses, kl_losses, gradient buffer).  beta None: the EXISTING entry of this form (adam False:
        forward_backward, which has no cache; vclip: mi_ppo_train_step_vclip); else mi_ppo_train_step_kl."""
        d, M = self.d, q.M
        a = (1.0 / M, 1.0, ALPHA)
        flat = form == "flat"
        data = (q.s, q.a, q.Rd, q.adv) if flat else (q.tab["s"], q.tab["a"], q.tab["R"], q.tab["adv"])
        lp, mo = ((q.lp, q.mo) if flat else (q.tab["lp"], q.tab["mo"])) if cached else (None, None)
        vo = (q.vo if flat else q.tab["vo"]) if vclip else None
        rows = None if flat else q.rows
        if beta is None:
            if vclip:
                d.train_step_vclip(comm, *data, lp, vo, EPS_V, rows, M, *a, adam=adam)
            elif not adam:
                assert flat and not cached
                d.forward_backward(*data, M, 1.0 / M, 1.0)
            elif comm is not None:
                d.train_step_dp(comm, *data, lp, rows, M, *a)
            elif flat:
                d.train_step(*data, M, *a, logp_old=lp)
            else:
                d.train_step_idx(*data, lp, rows, M, *a)
        else:
            d.train_step_kl(comm, *data, lp, mo, beta, rows, M, *a, adam=adam, old_values=vo, clip_range_vf=EPS_V if vclip else None)
        return [x.clone() for x in (d.params, d.adam_m, d.adam_v)], d.losses.clone(), d.kl_losses.clone(), d.grads.clone()


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


def kl_ok(got, ref_scal):
    return abs(float(got) - ref_scal["kl"]) <= ref_scal["bound"]


# ---- 1. the cache ----
@pytest.mark.parametrize("shape,precision,M", GRID)
def test_cache_keeps_the_means_and_the_log_probabilities(rigs, shape, precision, M):
    import torch
    r = rigs(shape, precision)
    q, d = r.problem(M), r.d
    want = torch.empty(M, device=d.device)
    d.logp_old(q.s, q.a, M, want)
    assert bitwise(q.lp.contiguous(), want)
    mean64 = kc.old_means(q.c)
    err = np.abs(q.mo_host - mean64).max()
    print("\n%s %s M = %d: old means, max abs error %.3e" % (shape, precision, M, err))
    assert np.allclose(q.mo_host, mean64, rtol=pc.ACT_RTOL, atol=pc.ACT_ATOL)
    assert bool((q.lp_buf[M:] == SENT).all()) and bool((q.mo_buf[M * r.A:] == SENT).all())
    # a second run gives the same bits
    lp2, mo2 = torch.empty(M, device=d.device), torch.empty(M, r.A, device=d.device)
    d.old_policy_cache(q.s, q.a, M, lp2, mo2)
    assert bitwise(lp2, want) and bitwise(mo2, q.mo.contiguous())


# ---- 2. beta = 0 measures and adds nothing ----
@pytest.mark.parametrize("shape,precision,M", GRID)
def test_beta_zero_is_the_existing_step(rigs, shape, precision, M):
    import torch
    r = rigs(shape, precision)
    q = r.problem(M)
    for form in ("flat", "idx"):
        for cached in (True, False):
            r.restore(q)
            want = r.step(q, form, cached=cached)
            r.restore(q)
            got = r.step(q, form, 0.0, cached=cached)
            tag = (shape, precision, M, form, cached)
            assert all(torch.equal(x, y) for x, y in zip(got[0], want[0])), tag
            assert torch.equal(got[1][:5], want[1][:5]) and torch.equal(got[1], want[1]), tag
            K = got[2].cpu().numpy()
            ref = q.ref["scal"] if not cached else kc.reference(q.c, 0.0, mean_old=q.mo_host)["scal"]
            assert kl_ok(K[0], ref) and K[1] == 0.0, (tag, K, ref["kl"])
    r.restore(q)
    want = r.step(q, "flat", cached=False, adam=False)
    assert bool((want[3][r.used] != 4.25).any())
    r.restore(q)
    got = r.step(q, "flat", 0.0, cached=False, adam=False)
    assert torch.equal(got[3][r.used], want[3][r.used]) and bitwise(got[0], q.state0)
    r.restore(q)


# ---- 3. beta = 0.7 against float64 ----
_REF = {}


def references(r, q):
    """(float64 reference with the cache's fp32 means, the fp32 oracle's own distance from float64 per gradient), once per (shape, precision, M)."""
    import torch
    key = (r.shape, r.precision, q.M)
    if key not in _REF:
        ref_c = kc.reference(q.c, kc.BETA, mean_old=q.mo_host)
        g32 = kc.reference(q.c, kc.BETA, dtype=torch.float32)["grads"]
        _REF[key] = (ref_c, {k: rel_err(g32[k], q.ref["grads"][k]) for k in g32})
    return _REF[key]


@pytest.mark.parametrize("form", ["flat", "idx"])
@pytest.mark.parametrize("shape,precision,M", GRID)
def test_penalised_step_against_float64(rigs, shape, precision, M, form):
    r = rigs(shape, precision)
    q = r.problem(M)
    ref_c, d32 = references(r, q)
    for cached, ref in ((True, ref_c), (False, q.ref)):
        r.restore(q)
        state, losses, K, _ = r.step(q, form, kc.BETA, cached=cached, adam=False)
        g = r.d.export_grads()
        L, K, s = losses.cpu().numpy(), K.cpu().numpy(), ref["scal"]
        print("\n%s %s M = %d %s cached = %s: KL %.9g (float64 %.9g, error %.2e, bound %.2e), loss rel %.2e" %
              (shape, precision, M, form, cached, K[0], s["kl"], abs(K[0] - s["kl"]), s["bound"], abs(L[3] - s["loss"]) / abs(s["loss"])))
        assert kl_ok(K[0], s)
        assert K[1].tobytes() == (np.float32(kc.BETA) * K[0]).astype(np.float32).tobytes()      # the penalty is beta32 x the KL slot, one fp32 product
        assert float(K[1]) == pytest.approx(s["penalty"], rel=pc.LOSS_REL, abs=kc.BETA32 * s["floor"])
        assert float(L[3]) == pytest.approx(s["loss"], rel=pc.LOSS_REL, abs=pc.LOSS_ABS)
        bound = {k: pc.GRAD_REL if precision == "fp32" else max(X3_GRAD_FLOOR, X3_GRAD_FACTOR * d32[k]) for k in kc.POLICY_NET}
        err = {k: rel_err(g[k], ref["grads"][k]) for k in kc.POLICY_NET}
        for k in kc.POLICY_NET:
            print("  %-28s %.3e of max (bound %.1e)" % (k, err[k], bound[k]))
        assert not {k: (err[k], bound[k]) for k in kc.POLICY_NET if err[k] > bound[k]}
        assert bitwise(state, q.state0)                                              # adam = 0 leaves the parameters and the optimiser state alone
        # the penalty really is in the gradient: without it the log-std gradient is elsewhere
        r.restore(q)
        _, losses_u, _, _ = r.step(q, form, 0.0, cached=cached, adam=False)
        g_u = r.d.export_grads()
        assert rel_err(g_u["policy/action_logstd"], ref["grads"]["policy/action_logstd"]) > 10 * bound["policy/action_logstd"]
        if precision == "fp32":                                                      # nothing on the value side, and none of the other scalars, changes
            for k in kc.VALUE_NET:
                assert np.array_equal(g[k].view(np.int32), g_u[k].view(np.int32)), k
            Lu = losses_u.cpu().numpy()
            assert all(L[i].tobytes() == Lu[i].tobytes() for i in (0, 1, 2, 4)) and np.array_equal(L[5:].view(np.int32), Lu[5:].view(np.int32))
    # the step from the cache against the step that evaluates the old policy itself
    r.restore(q)
    from_cache = r.step(q, form, kc.BETA, cached=True)
    r.restore(q)
    in_step = r.step(q, form, kc.BETA, cached=False)
    diff = float((from_cache[0][0] - in_step[0][0]).abs().max())
    print("  parameters, cache against in-step old policy: max abs difference %.3e, bitwise %s" % (diff, bitwise(from_cache[0], in_step[0])))
    assert diff <= 1e-7
    assert not bitwise(from_cache[0][0], q.state0[0])
    r.restore(q)


# ---- 4. theta == theta_old ----
@pytest.mark.parametrize("shape,precision,M", GRID)
def test_kl_of_a_policy_with_itself(rigs, shape, precision, M):
    import torch
    r = rigs(shape, precision)
    q, d = r.problem(M), r.d
    d.update_old()
    lp, mo = torch.empty(M, device=d.device), torch.empty(M, r.A, device=d.device)
    d.old_policy_cache(q.s, q.a, M, lp, mo)
    for cached in (False, True):
        d.grads.fill_(4.25)
        if cached:
            d.train_step_kl(None, q.s, q.a, q.Rd, q.adv, lp, mo, kc.BETA, None, M, 1.0 / M, 1.0, ALPHA, adam=False)
        else:
            d.train_step_kl(None, q.s, q.a, q.Rd, q.adv, None, None, kc.BETA, None, M, 1.0 / M, 1.0, ALPHA, adam=False)
        K = d.kl_losses.cpu().numpy()
        print("\n%s %s M = %d cached = %s: KL(theta || theta) = %.3e" % (shape, precision, M, cached, K[0]))
        assert 0.0 <= K[0] <= 1e-10 and 0.0 <= K[1] <= 1e-10
    r.restore(q)


# ---- 5. combinations ----
@pytest.mark.parametrize("form", ["flat", "idx"])
@pytest.mark.parametrize("shape,precision,M", GRID)
def test_combinations(rigs, recording_comm, shape, precision, M, form):
    import torch
    r = rigs(shape, precision)
    q, d = r.problem(M), r.d
    # with old values: the value side is mi_ppo_train_step_vclip's, the policy side the KL step's without them
    r.restore(q)
    r.step(q, form, kc.BETA, adam=False, vclip=True)
    g_both, L_both, K_both = d.export_grads(), d.losses.clone(), d.kl_losses.clone()
    r.restore(q)
    r.step(q, form, None, adam=False, vclip=True)
    g_v, L_v = d.export_grads(), d.losses.clone()
    r.restore(q)
    r.step(q, form, kc.BETA, adam=False)
    g_k, L_k, K_k = d.export_grads(), d.losses.clone(), d.kl_losses.clone()
    for k in kc.VALUE_NET:
        assert np.array_equal(g_both[k].view(np.int32), g_v[k].view(np.int32)), k
    for k in kc.POLICY_NET:
        assert np.array_equal(g_both[k].view(np.int32), g_k[k].view(np.int32)), k
    assert bitwise(L_both[1:2], L_v[1:2]) and bitwise(L_both[[0, 2, 4]], L_k[[0, 2, 4]]) and bitwise(K_both, K_k)
    assert not bitwise(L_both[1:2], L_k[1:2])                                        # (the planned old values do clip)
    # twice the same
    r.restore(q)
    first = r.step(q, form, kc.BETA)
    r.restore(q)
    again = r.step(q, form, kc.BETA)
    assert all(bitwise(x, y) for x, y in zip(first, again))
    # on a recording communicator: adam = 0 followed by mi_ppo_apply_adam
    r.restore(q)
    dp = r.step(q, form, kc.BETA, comm=recording_comm)
    r.restore(q)
    r.step(q, form, kc.BETA, adam=False)
    d.apply_adam(ALPHA)
    assert bitwise([d.params, d.adam_m, d.adam_v], dp[0]) and bitwise(dp[1], first[1]) and bitwise(dp[2], first[2])
    # with clipping by the global norm: "gradient buffer x factor in fp32, then mi_ppo_apply_adam"
    r.restore(q)
    d.set_max_grad_norm(0.5)
    clipped = r.step(q, form, kc.BETA)
    rec = d.grad_clip.clone()
    assert rec[2].item() == 0.5 and 0.0 < rec[1].item() <= 1.0 and rec[0].item() > 0.0
    r.restore(q)
    r.step(q, form, kc.BETA, adam=False)
    d.grads.mul_(rec[1])
    d.apply_adam(ALPHA)
    assert bitwise([d.params, d.adam_m, d.adam_v], clipped[0]), (shape, precision, M, form, rec)
    assert torch.equal(clipped[1], first[1]) and torch.equal(clipped[2], first[2])
    r.restore(q)


# ---- 6. refusals ----
def test_refusals_leave_everything_alone(rigs):
    import torch
    from mi355 import lib as milib
    r = rigs("A3", "fp32")
    q, d = r.problem(5), r.d
    M = 5
    a = (1.0 / M, 1.0, ALPHA)

    def untouched():
        return bitwise([d.params, d.adam_m, d.adam_v], q.state0) and bool((d.grads == 4.25).all())
    with pytest.raises(milib.MiError, match=r"mi_ppo_train_step_kl failed \(-1\).*logp_old and mean_old come together"):
        d.train_step_kl(None, q.s, q.a, q.Rd, q.adv, q.lp, None, kc.BETA, None, M, *a)
    with pytest.raises(milib.MiError, match=r"mi_ppo_train_step_kl failed \(-1\).*logp_old and mean_old come together"):
        d.train_step_kl(None, q.s, q.a, q.Rd, q.adv, None, q.mo, kc.BETA, None, M, *a)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(milib.MiError, match=r"mi_ppo_train_step_kl failed \(-1\).*kl_coef"):
            d.train_step_kl(None, q.s, q.a, q.Rd, q.adv, q.lp, q.mo, bad, None, M, *a)
    with pytest.raises(milib.MiError, match=r"mi_ppo_train_step_kl failed \(-1\).*adam is 0"):
        d.L.mi_ppo_train_step_kl(d.handle, None, d.stream(), q.s.data_ptr(), q.a.data_ptr(), q.Rd.data_ptr(), q.adv.data_ptr(), q.lp.data_ptr(), q.mo.data_ptr(), kc.BETA,
                                 None, 0.0, None, 0, M, 1.0 / M, 1.0, 2, ALPHA, 0.9, 0.999, 1e-8)
    with pytest.raises(milib.MiError, match=r"mi_ppo_train_step_kl failed \(-1\).*clip_range_vf"):
        d.train_step_kl(None, q.s, q.a, q.Rd, q.adv, q.lp, q.mo, kc.BETA, None, M, *a, old_values=q.vo, clip_range_vf=0.0)
    with pytest.raises(milib.MiError, match=r"mi_ppo_train_step_kl failed \(-1\).*batch outside"):
        d.L.mi_ppo_train_step_kl(d.handle, None, d.stream(), q.s.data_ptr(), q.a.data_ptr(), q.Rd.data_ptr(), q.adv.data_ptr(), None, None, kc.BETA, None, 0.0, None, 0,
                                 d.max_batch + 1, 1.0 / M, 1.0, 1, ALPHA, 0.9, 0.999, 1e-8)
    assert untouched()
    sums = torch.zeros(4, dtype=torch.float64, device=d.device)
    with pytest.raises(milib.MiError, match=r"mi_ppo_kl_stats_idx failed \(-1\).*accumulate"):
        d.L.mi_ppo_kl_stats_idx(d.handle, d.stream(), q.tab["s"].data_ptr(), q.tab["mo"].data_ptr(), q.rows.data_ptr(), int(q.tab["s"].shape[0]), M, 2,
                                sums.data_ptr(), sums.data_ptr())
    with pytest.raises(milib.MiError, match=r"mi_ppo_kl_stats_idx failed \(-1\).*missing buffers"):
        d.L.mi_ppo_kl_stats_idx(d.handle, d.stream(), q.tab["s"].data_ptr(), None, q.rows.data_ptr(), int(q.tab["s"].shape[0]), M, 0, sums.data_ptr(), sums.data_ptr())
    assert untouched()
    r.restore(q)


@pytest.mark.parametrize("name", pc.PER_LAYER_CASES[::2])
def test_no_per_layer_form(name):
    """An engine outside the fused kernels' range refuses the penalised step, the cache and the statistics pass with MI_ERR_SHAPE and writes nothing."""
    import torch
    from mi355 import lib as milib
    from mi355.ppo_device import PpoDevice
    din, A, hidden, M, _, _ = pc.ENGINE_CASES[name]
    low, high = pc.bounds(A)
    d = PpoDevice(din, A, low, high, pc.EPS, pc.VALUE_SCALE, pc.ENTROPY_SCALE, hidden=hidden, max_batch=32)
    assert not d.fused_ok()
    M = min(M, 32)
    z = lambda *s: torch.zeros(*s, device=d.device)      # noqa: E731
    d.params.normal_(); d.adam_m.fill_(0.5); d.adam_v.fill_(0.25); d.grads.fill_(4.25)
    before = [x.clone() for x in (d.params, d.adam_m, d.adam_v, d.grads)]
    lp, mo = torch.full((M,), SENT, device=d.device), torch.full((M, A), SENT, device=d.device)
    with pytest.raises(milib.MiError, match=r"mi_ppo_train_step_kl failed \(-2\).*no per-layer form"):
        d.train_step_kl(None, z(M, din), z(M, A), z(M), z(M), None, None, kc.BETA, None, M, 1.0 / M, 1.0, ALPHA)
    with pytest.raises(milib.MiError, match=r"mi_ppo_old_policy_cache failed \(-2\)"):
        d.old_policy_cache(z(M, din), z(M, A), M, lp, mo)
    sums = torch.full((4,), 7.0, dtype=torch.float64, device=d.device)
    with pytest.raises(milib.MiError, match=r"mi_ppo_kl_stats_idx failed \(-2\)"):
        d.kl_stats(z(M, din), z(M, A), torch.arange(M, dtype=torch.int32, device=d.device), M, sums, torch.zeros(8, dtype=torch.float64, device=d.device))
    assert bitwise([d.params, d.adam_m, d.adam_v, d.grads], before) and bool((lp == SENT).all()) and bool((mo == SENT).all()) and bool((sums == 7.0).all())
    d.close()


# ---- 7. the statistics pass ----
@pytest.mark.parametrize("shape,precision,M", GRID)
def test_kl_stats_pass(rigs, shape, precision, M):
    import torch
    from mi355.ppo_device import N_KL_STATS, kl_stats_summary
    r = rigs(shape, precision)
    q, d = r.problem(M), r.d
    n = q.tab["s"].shape[0]
    f64 = lambda k, v=0.0: torch.full((k,), v, dtype=torch.float64, device=d.device)      # noqa: E731
    assert d.kl_stats_scratch_doubles(M) == N_KL_STATS * ((M + 31) // 32)
    losses_before, kl_before = d.losses.clone(), d.kl_losses.clone()

    def run(states, mo, rows, m, stats, accumulate=False):
        d.kl_stats(states, mo, rows, m, stats, f64(d.kl_stats_scratch_doubles(m), -1.0), accumulate=accumulate)
        return stats.cpu().numpy().copy()
    got = run(q.tab["s"], q.tab["mo"], q.rows, M, f64(N_KL_STATS, 7.0))
    # float64 on the very fp32 old means the kernel read
    ref = kc.reference(q.c, 0.0, mean_old=q.mo_host)
    want = np.array([M, ref["kl_m"].sum(), (ref["kl_m"] ** 2).sum(), ref["mean_part_m"].sum()])
    s = kl_stats_summary(got)
    print("\n%s %s M = %d: sums %s, float64 %s; kl %.9g kl_std %.3e mean part %.3e" % (shape, precision, M, got, want, s["kl"], s["kl_std"], s["kl_mean_part"]))
    assert got[0] == M and s["samples"] == M
    assert s["kl"] == pytest.approx(want[1] / M, rel=1e-4) and got[2] == pytest.approx(want[2], rel=2e-4) and s["kl_mean_part"] == pytest.approx(want[3] / M, rel=1e-4)
    assert s["kl_std"] == pytest.approx(ref["kl_m"].std(), rel=1e-4)
    assert run(q.tab["s"], q.tab["mo"], q.rows, M, f64(N_KL_STATS)).tobytes() == got.tobytes()      # run to run
    # NaN in the rows that are not named changes nothing: the same samples as tables of exactly M rows
    dense = run(q.s, q.mo.contiguous(), torch.arange(M, dtype=torch.int32, device=d.device), M, f64(N_KL_STATS))
    assert dense.tobytes() == got.tobytes()
    assert bool(torch.isnan(q.tab["mo"]).any())
    # two chunks with accumulate
    cut = max(1, M // 3)
    acc = f64(N_KL_STATS)
    run(q.tab["s"], q.tab["mo"], q.rows[:cut].contiguous(), cut, acc)
    chunked = run(q.tab["s"], q.tab["mo"], q.rows[cut:].contiguous(), M - cut, acc, accumulate=True)
    assert chunked[0].tobytes() == got[0].tobytes() and np.all(np.abs(chunked[1:] - got[1:]) <= 1e-12 * np.abs(got[1:]))
    # nothing of the training state is written
    assert bitwise([d.params, d.adam_m, d.adam_v], q.state0) and bool((d.grads == 4.25).all()) and bitwise(d.losses, losses_before) and bitwise(d.kl_losses, kl_before)
    # theta == theta_old: the KL is exactly zero (the pass spells its means as the cache does)
    d.update_old()
    lp, mo = torch.empty(M, device=d.device), torch.empty(M, r.A, device=d.device)
    d.old_policy_cache(q.s, q.a, M, lp, mo)
    zero = run(q.s, mo, torch.arange(M, dtype=torch.int32, device=d.device), M, f64(N_KL_STATS, 7.0))
    assert zero.tolist() == [float(M), 0.0, 0.0, 0.0]
    r.restore(q)


# ---- 8. PPO.train ----
def test_ppo_train_with_the_penalty_on(tmp_path):
    import torch
    from ppo import ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON, _adam_alpha
    rng = np.random.RandomState(9)
    M = 24
    s, a = rng.standard_normal((M, 67)).astype(np.float32), rng.uniform(0, 1, (M, 2)).astype(np.float32)
    R, adv = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M).astype(np.float32)
    _, m1 = make_pair(tmp_path / "a")
    _, m2 = make_pair(tmp_path / "b")
    _, m3 = make_pair(tmp_path / "c")
    for m in (m1, m2, m3):                                                           # a policy away from its old one
        m.train(s, a, R, adv)
    assert bitwise(flat_state(m1), flat_state(m2))
    m1.set_kl_penalty(kc.BETA)
    out = m1.train_step(s, a, R, adv)
    up = lambda x: torch.from_numpy(x).to(m2.dev.device)      # noqa: E731
    m2.dev.train_step_kl(None, up(s), up(a), up(R), up(adv), None, None, kc.BETA, None, M, 1.0 / M, 1.0,
                         _adam_alpha(m2.current_learning_rate(), m2.beta1_power, m2.beta2_power), ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON)
    assert bitwise(flat_state(m1), flat_state(m2))
    K, L = m2.dev.kl_losses.cpu().numpy(), m2.dev.losses.cpu().numpy()
    assert set(out) == {"policy_loss", "value_loss", "entropy_loss", "loss", "prob_ratio", "kl", "kl_penalty"}
    assert out["kl"] == float(K[0]) > 0.0 and out["kl_penalty"] == float(K[1]) > 0.0 and out["loss"] == float(L[3])
    out3 = m3.train_step(s, a, R, adv)
    assert set(out3) == set(out) - {"kl", "kl_penalty"} and not bitwise(flat_state(m3), flat_state(m1))
    assert out3["loss"] + out["kl_penalty"] == pytest.approx(out["loss"], rel=1e-5, abs=1e-6)


# ---- 9. the rollout buffers ----
SEED = 3


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return make_world(tmp_path_factory, "kl_penalty", policy=False)


def collect(world, tmp, continuous, E, T, source):
    """A policy and a full E x T collection through the buffer's own step; the device tables are those of the first collection of this (class, E, T) (the recording
    step's split-K layers end in fp32 atomics).  continuous: lane 1 reports a done at its step 3."""
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


def measured_kl(buf, m):
    import torch
    from mi355.ppo_device import N_KL_STATS, kl_stats_summary
    valid = torch.from_numpy(buf.rows.valid_rows()).to(buf.device)
    n = int(valid.numel())
    sums = torch.zeros(N_KL_STATS, dtype=torch.float64, device=buf.device)
    m.dev.kl_stats(buf.states, buf.mean_old, valid, n, sums, torch.zeros(m.dev.kl_stats_scratch_doubles(n), dtype=torch.float64, device=buf.device))
    return kl_stats_summary(sums.cpu().numpy())


@pytest.mark.parametrize("continuous", [False, True])
@pytest.mark.parametrize("E,T,batch", [(3, 5, 4), (5, 20, 32)])
def test_rollout_buffer_update_end_to_end(world, tmp_path, continuous, E, T, batch):
    import torch
    from ppo import ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON, _adam_alpha
    EPOCHS, BETA0 = 2, 0.5
    source = []
    # the parent's behaviour: a policy whose setter is never called
    m0, b0 = collect(world, tmp_path / "w0", continuous, E, T, source)
    assert m0.kl_penalty is None
    out0 = b0.update(num_epochs=EPOCHS, batch_size=batch)
    assert b0.mean_old is None and not ({"kl", "kl_coef", "kl_coef_next", "kl_adapted"} & set(out0)) and "kl" not in out0["losses"][0]
    # the penalty on, fixed coefficient
    m1, b1 = collect(world, tmp_path / "w1", continuous, E, T, source)
    m1.set_kl_penalty(BETA0)
    times = {}
    out1 = b1.update(num_epochs=EPOCHS, batch_size=batch, stage_times=times)
    assert set(out1) == set(out0) | {"kl", "kl_coef", "kl_coef_next", "kl_adapted"} and "kl_stats" in times
    assert out1["kl_coef"] == BETA0 == out1["kl_coef_next"] == m1.kl_penalty and out1["kl_adapted"] is False
    n_valid = out1["samples"]
    assert n_valid % batch != 0                                                      # the last minibatch of an epoch is partial
    assert out1["kl"] == measured_kl(b1, m1) and out1["kl"]["samples"] == n_valid and out1["kl"]["kl"] > 0.0
    # a host loop on a twin: the cache, then one train_step_kl per minibatch
    _, m2 = make_pair(tmp_path / "w2")
    m2.update_old_policy()
    valid = b1.rows.valid_rows()
    lp2, mo2 = torch.zeros_like(b1.logp_old), torch.zeros_like(b1.mean_old)
    m2.dev.old_policy_cache(b1.states, b1.actions, b1.n_table_rows, lp2, mo2)
    idx = torch.from_numpy(valid).to(b1.device).long()
    assert bitwise(lp2[idx], b1.logp_old[idx]) and bitwise(mo2[idx], b1.mean_old[idx])
    np.random.seed(SEED)
    b1p, b2p = np.float32(ADAM_BETA1), np.float32(ADAM_BETA2)
    records, kls = [], []
    for _ in range(EPOCHS):
        indices = np.arange(len(valid))
        np.random.shuffle(indices)
        perm = torch.from_numpy(valid[indices]).to(b1.device)
        for i in range(0, len(valid), batch):
            mb = perm[i:i + batch]
            k = int(mb.numel())
            m2.dev.train_step_kl(None, b1.states, b1.actions, b1.returns, b1.advantages, lp2, mo2, BETA0, mb, k, 1.0 / k, 1.0,
                                 _adam_alpha(m2.current_learning_rate(), b1p, b2p), ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON)
            records.append(m2.dev.losses.clone())
            kls.append(m2.dev.kl_losses.clone())
            b1p, b2p = np.float32(b1p * np.float32(ADAM_BETA1)), np.float32(b2p * np.float32(ADAM_BETA2))
    assert bitwise(flat_state(m2), flat_state(m1))
    rec, kl = torch.stack(records).cpu().numpy().astype(np.float64), torch.stack(kls).cpu().numpy().astype(np.float64)
    assert len(out1["losses"]) == len(rec)
    for i, x in enumerate(out1["losses"]):
        assert [x["policy_loss"], x["value_loss"], x["entropy_loss"], x["loss"], x["prob_ratio"]] == list(rec[i, :5]) and [x["kl"], x["kl_penalty"]] == list(kl[i])
    assert out1["losses"][0]["kl"] <= 1e-10 and out1["losses"][-1]["kl"] > 0.0      # the first step starts at theta_old
    assert not bitwise(flat_state(m1), flat_state(m0))
    # the rule, for a target below, inside and above the measured KL; the second update uses the new coefficient
    kl1 = out1["kl"]["kl"]
    for j, (target, factor) in enumerate(((kl1 / 4.0, 2.0), (kl1, 1.0), (kl1 * 4.0, 0.5))):
        m, b = collect(world, tmp_path / ("t%d" % j), continuous, E, T, source)
        m.set_kl_penalty(BETA0, target=target)
        out = b.update(num_epochs=EPOCHS, batch_size=batch)
        assert bitwise(flat_state(m), flat_state(m1)) and out["kl"] == out1["kl"] and out["losses"] == out1["losses"]
        assert out["kl_coef"] == BETA0 and out["kl_coef_next"] == BETA0 * factor == m.kl_penalty == kc.adapted(BETA0, target, kl1) and out["kl_adapted"] is True
        np.random.seed(SEED + 1)
        nxt = b.update(num_epochs=1, batch_size=batch)
        assert nxt["kl_coef"] == BETA0 * factor
        beta32 = np.float32(BETA0 * factor)
        for x in nxt["losses"][1:]:
            assert np.float32(x["kl_penalty"]).tobytes() == (beta32 * np.float32(x["kl"])).astype(np.float32).tobytes() and x["kl"] > 0.0
        st = m.kl_penalty_state()
        assert st["kl_target"] == target and st["kl_coef"] == nxt["kl_coef_next"]
    # switched on and off again: the parent's keys and parameters
    m4, b4 = collect(world, tmp_path / "w4", continuous, E, T, source)
    m4.set_kl_penalty(BETA0, target=0.01)
    m4.set_kl_penalty(None)
    out4 = b4.update(num_epochs=EPOCHS, batch_size=batch)
    assert set(out4) == set(out0) and out4["losses"] == out0["losses"] and bitwise(flat_state(m4), flat_state(m0)) and b4.mean_old is None
    # with value clipping, diagnostics and a KL stop
    m5, b5 = collect(world, tmp_path / "w5", continuous, E, T, source)
    m5.set_kl_penalty(BETA0, target=0.01)
    m5.set_value_clip(EPS_V)
    out5 = b5.update_with_diagnostics(num_epochs=EPOCHS, batch_size=batch, target_kl=1e-9)
    assert out5["stopped_early"] and out5["epochs_run"] == 1 and "value_clip_fraction" in out5["epochs"][0] and out5["kl"]["kl"] > 0.0 and out5["kl_adapted"] is True
    assert len(out5["losses"]) == -(-n_valid // batch) and all("kl" in x for x in out5["losses"])
    # the state round trip: a policy that loads the state continues bit for bit
    m6, b6 = collect(world, tmp_path / "w6", continuous, E, T, source)
    m6.load_kl_penalty_state({"kl_coef": BETA0, "kl_target": None})
    out6 = b6.update(num_epochs=EPOCHS, batch_size=batch)
    assert bitwise(flat_state(m6), flat_state(m1)) and out6["losses"] == out1["losses"] and m6.kl_penalty_state() == m1.kl_penalty_state()


def test_a_policy_outside_the_fused_kernels_is_refused_before_any_launch(world, tmp_path, monkeypatch):
    import torch
    m, buf = collect(world, tmp_path / "w", False, 3, 5, [])
    m.set_kl_penalty(0.5)
    monkeypatch.setattr(m.dev, "fused_ok", lambda: False)
    before = [x.clone() for x in (buf.returns, buf.advantages, buf.logp_old, m.dev.params, m.dev.params_old)]
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match="KL penalty"):
        buf.update(num_epochs=1, batch_size=4)
    assert all(torch.equal(x, y) for x, y in zip((buf.returns, buf.advantages, buf.logp_old, m.dev.params, m.dev.params_old), before))
    assert np.array_equal(np.random.get_state()[1], state)
    with pytest.raises(ValueError, match="KL penalty needs the fused one-call step"):
        m.train(np.zeros((4, 67), np.float32), np.zeros((4, 2), np.float32), np.zeros(4, np.float32), np.zeros(4, np.float32))
