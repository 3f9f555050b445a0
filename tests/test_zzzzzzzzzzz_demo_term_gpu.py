"""The PPO step with a demonstration term (mi_ppo_train_step_demo, PpoDevice.train_step_demo, PPO.set_demonstration_loss / _demo_rows,
RolloutBuffer.set_demonstrations) on the GPU.  Problems, the float64 reference and the bounds are those of tests/demo_term_cases.py:
  the PPO scalars and mean_sq_error 1e-4 relative; demo_loss 1e-4 of its absolute terms; the KL by kl_penalty_cases.kl_bound; the total loss 1e-4 of the sum of the
  absolute values of its terms; gradients 2e-4 of each tensor's maximum in fp32 and max(1e-3, 4 x the fp32 reference's distance) in bf16x3; parameters behind one
  step within 2e-6 of TF-Adam on the device's own gradients (entries whose gradient is above 1e-3 of the tensor's maximum, as tests/behaviour_cloning_cases.py).
Every measured distance is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import behaviour_cloning_cases as bc  # noqa: E402
import demo_term_cases as dc  # noqa: E402
from rollout_gpu_common import bitwise, flat_state, make_pair  # noqa: E402

ALPHA = 1e-4
FILL = 4.25
GRID = [(s, p, mp, md) for s in ("A2", "A3") for p in ("fp32", "bf16x3") for mp, md in dc.COUNTS]


class Problem:
    pass


class Rig:
    """One engine per (shape, precision) and its problems per (M_p, M_d): contiguous tensors, and the same samples as shuffled rows of NaN-filled tables on both sides."""

    def __init__(self, shape, precision):
        import torch
        from mi355.ppo_device import PpoDevice
        self.shape, self.precision = shape, precision
        self.din, self.A, self.hidden = dc.SHAPES[shape][:3]
        low, high = dc.pc.bounds(self.A)
        self.d = PpoDevice(self.din, self.A, low, high, dc.pc.EPS, dc.pc.VALUE_SCALE, dc.pc.ENTROPY_SCALE, hidden=self.hidden, max_batch=320, precision=precision,
                           wide_inputs=1 if self.din > 96 else 0)
        assert self.d.fused_ok()
        self.o7 = self.d.layout[dc.NAMES[7]][0]            # where the value net starts in the flat buffers
        self.used = torch.zeros(self.d.n_flat, dtype=torch.bool, device=self.d.device)
        for _, (o_, s_) in self.d.layout.items():
            self.used[o_:o_ + s_] = True
        self.problems = {}

    def restore(self, q):
        d = self.d
        for x, y in zip((d.params, d.adam_m, d.adam_v, d.params_old), q.state0 + [q.old]):
            x.copy_(y)
        d.grads.fill_(FILL)
        d.set_max_grad_norm(None)

    def up(self, x):
        import torch
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.d.device)

    def problem(self, Mp, Md):
        import torch
        key = (Mp, Md)
        if key in self.problems:
            self.restore(self.problems[key])
            return self.problems[key]
        d, A = self.d, self.A
        q = Problem()
        q.Mp, q.Md, q.c = Mp, Md, dc.case(self.shape, Mp, Md)
        c = q.c
        rng = np.random.RandomState(900 + 10 * Mp + Md)
        d.load_params(c.theta, dc.pc.old_names(c.theta_old))
        q.m0 = {k: (0.01 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in c.theta.items()}
        q.v0 = {k: ((0.01 * rng.standard_normal(v.shape)) ** 2 + 1e-6).astype(np.float32) for k, v in c.theta.items()}
        d.load_slots(q.m0, q.v0)
        q.state0, q.old = [x.clone() for x in (d.params, d.adam_m, d.adam_v)], d.params_old.clone()
        q.s, q.a, q.R, q.adv, q.vo, q.ds, q.da = (self.up(x) for x in (c.s, c.a, c.R, c.adv, c.v_old, c.ds, c.da))
        q.lp, q.mo = torch.zeros(Mp, device=d.device), torch.zeros(Mp, A, device=d.device)
        d.old_policy_cache(q.s, q.a, Mp, q.lp, q.mo)       # the caches the steps read: log pi_old and the old means of the PPO rows
        n, nd = 2 * Mp + 3, 2 * Md + 5
        q.rows = torch.from_numpy(rng.permutation(n)[:Mp].astype(np.int32)).to(d.device)
        q.drows = torch.from_numpy(rng.permutation(nd)[:Md].astype(np.int32)).to(d.device)
        q.tab = {}
        for name, x, rows, total in (("s", q.s, q.rows, n), ("a", q.a, q.rows, n), ("R", q.R, q.rows, n), ("adv", q.adv, q.rows, n), ("vo", q.vo, q.rows, n),
                                     ("lp", q.lp, q.rows, n), ("mo", q.mo, q.rows, n), ("ds", q.ds, q.drows, nd), ("da", q.da, q.drows, nd)):
            t = torch.full((total,) + tuple(x.shape[1:]), float("nan"), device=d.device)      # NaN in every row no list names, in every table of both sides
            t[rows.long()] = x
            q.tab[name] = t
        self.problems[key] = q
        self.restore(q)
        return q

    def step(self, q, form, variant, kind, coef=dc.C_D, adam=True, comm=None, cache=True):
        """One demonstration step from the state the engine is in -> (params / m / v, losses, kl, demo scalars, gradient buffer, dv)."""
        d = self.d
        vclip, kl = dc.VARIANTS[variant]
        g = (lambda k: getattr(q, k)) if form == "flat" else (lambda k: q.tab[k])
        d.train_step_demo(comm, g("s"), g("a"), g("R"), g("adv"), g("lp") if cache else None, g("mo") if cache and kl else None, dc.BETA if kl else None,
                          None if form == "flat" else q.rows, q.Mp, g("ds"), g("da"), None if form == "flat" else q.drows, q.Md, kind, coef, 1.0 / q.Md,
                          1.0 / q.Mp, 1.0, ALPHA, adam=adam, old_values=g("vo") if vclip else None, clip_range_vf=dc.EPS_V if vclip else None)
        return ([x.clone() for x in (d.params, d.adam_m, d.adam_v)], d.losses.clone(), d.kl_losses.clone(), d.demo_losses.clone(), d.grads.clone(),
                d.value_head_grad[:q.Mp + q.Md].clone())

    def existing(self, q, variant, adam, cache=True):
        """The matching existing entry on the PPO rows alone (contiguous) -> (params / m / v, losses, gradient buffer)."""
        d = self.d
        vclip, kl = dc.VARIANTS[variant]
        lp, mo = (q.lp, q.mo) if cache else (None, None)
        if kl:
            d.train_step_kl(None, q.s, q.a, q.R, q.adv, lp, mo, dc.BETA, None, q.Mp, 1.0 / q.Mp, 1.0, ALPHA, adam=adam, old_values=q.vo if vclip else None,
                            clip_range_vf=dc.EPS_V if vclip else None)
        elif vclip:
            d.train_step_vclip(None, q.s, q.a, q.R, q.adv, lp, q.vo, dc.EPS_V, None, q.Mp, 1.0 / q.Mp, 1.0, ALPHA, adam=adam)
        elif adam:
            d.train_step(q.s, q.a, q.R, q.adv, q.Mp, 1.0 / q.Mp, 1.0, ALPHA, logp_old=lp)
        else:
            assert not cache                                # (mi_ppo_forward_backward evaluates the old policy itself)
            d.forward_backward(q.s, q.a, q.R, q.adv, q.Mp, 1.0 / q.Mp, 1.0)
        return [x.clone() for x in (d.params, d.adam_m, d.adam_v)], d.losses.clone(), d.grads.clone()


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


def check_against_float64(r, q, form, variant, kind):
    import torch
    d, tag = r.d, (r.shape, r.precision, q.Mp, q.Md, form, variant, kind)
    vclip, kl = dc.VARIANTS[variant]
    ref = dc.ref_of(r.shape, q.Mp, q.Md, variant, kind)
    scal, g64 = ref["scal"], ref["grads"]
    r.restore(q)
    state, losses, klv, demo, gbuf, dv = r.step(q, form, variant, kind, adam=False)
    g, L, D, K = d.export_grads(), losses.cpu().numpy(), demo.cpu().numpy(), klv.cpu().numpy()
    floor = scal["abs_terms"]
    print("\n%s: policy %.9g (%.9g) value %.9g (%.9g) entropy %.9g (%.9g) ratio %.9g (%.9g) loss %.9g (%.9g); demo_loss %.9g (float64 %.9g, error %.2e of the "
          "absolute terms), mean_sq_error %.9g (%.9g, rel %.2e)" %
          (tag, L[0], scal["policy_loss"], L[1], scal["value_loss"], L[2], scal["entropy_loss"], L[4], scal["ratio_mean"], L[3], scal["loss"], D[0], scal["demo_loss"],
           abs(float(D[0]) - scal["demo_loss"]) / floor, D[2], scal["mean_sq_error"], abs(float(D[2]) - scal["mean_sq_error"]) / scal["mean_sq_error"]))
    for i, k in ((0, "policy_loss"), (1, "value_loss"), (2, "entropy_loss"), (4, "ratio_mean")):
        assert float(L[i]) == pytest.approx(scal[k], rel=dc.LOSS_REL), (tag, k)
    assert abs(float(D[0]) - scal["demo_loss"]) <= dc.LOSS_REL * floor, tag
    assert float(D[2]) == pytest.approx(scal["mean_sq_error"], rel=dc.LOSS_REL), tag
    assert D[1].tobytes() == (np.float32(dc.C_D) * D[0]).astype(np.float32).tobytes(), tag
    terms = abs(scal["policy_loss"]) + abs(scal["value_loss"]) + abs(scal["entropy_loss"]) + dc.C_D32 * floor + (abs(scal["penalty"]) if kl else 0.0)
    assert abs(float(L[3]) - scal["loss"]) <= dc.LOSS_REL * terms, tag
    if kl:
        print("  kl %.9g (float64 %.9g, bound %.2e)" % (K[0], scal["kl"], scal["bound"]))
        assert abs(float(K[0]) - scal["kl"]) <= scal["bound"], tag
    # the mean action_mean is over the PPO rows alone
    assert np.abs(L[5:5 + r.A] - ref["mean"].mean(0)).max() <= dc.LOSS_REL * np.abs(ref["mean"]).mean(0).max() + 1e-6, tag
    g32 = dc.ref_of(r.shape, q.Mp, q.Md, variant, kind, torch.float32)["grads"] if r.precision != "fp32" else None
    bound = {k: dc.GRAD_REL if r.precision == "fp32" else max(dc.X3_GRAD_FLOOR, dc.X3_GRAD_FACTOR * dc.rel_err(g32[k], g64[k])) for k in dc.NAMES}
    err = {k: dc.rel_err(g[k], g64[k]) for k in dc.NAMES}
    for k in dc.NAMES:
        print("  %-28s %.3e of max (bound %.1e)" % (k, err[k], bound[k]))
    assert not {k: (err[k], bound[k]) for k in dc.NAMES if err[k] > bound[k]}, tag
    assert bitwise(state, q.state0), tag                    # adam = 0 leaves the parameters and the optimiser state alone
    assert bool((gbuf[r.used] != FILL).all()), tag
    # demonstration rows: dv exactly 0.0
    assert bool((dv[q.Mp:] == 0.0).all()) and bool((dv[:q.Mp] != 0.0).any()), tag
    # adam = 1: TF-Adam on the device's own gradients, from the non-zero slots
    r.restore(q)
    r.step(q, form, variant, kind, adam=True)
    p1 = d.export_params()
    worst = 0.0
    for k in dc.NAMES:
        want, _, _ = bc.adam_tf(q.c.theta[k], q.m0[k], q.v0[k], g[k], np.float32(ALPHA))
        big = np.abs(g[k]) > dc.ADAM_GMIN * np.abs(g[k]).max()
        dist = float(np.abs(p1[k].astype(np.float64) - want)[big].max())
        worst = max(worst, dist)
        assert big.any() and dist <= dc.ADAM_ABS, (tag, k, dist)
    print("  parameters behind the step: %.3e from TF-Adam on the device's gradients (bound %.1e)" % (worst, dc.ADAM_ABS))
    r.restore(q)


@pytest.mark.parametrize("form", ["flat", "idx"])
@pytest.mark.parametrize("shape,precision,Mp,Md", GRID)
def test_demo_step_against_float64(rigs, shape, precision, Mp, Md, form):
    r = rigs(shape, precision)
    q = r.problem(Mp, Md)
    for variant in dc.VARIANTS:
        for kind in dc.KINDS:
            check_against_float64(r, q, form, variant, kind)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_wide_inputs_against_float64(rigs, precision):
    r = rigs("W", precision)
    q = r.problem(33, 7)
    for form in ("flat", "idx"):
        for variant, kind in (("plain", "nll"), ("kl_vclip", "mse")):
            check_against_float64(r, q, form, variant, kind)


@pytest.mark.parametrize("shape,precision,Mp,Md", GRID)
def test_identities(rigs, recording_comm, shape, precision, Mp, Md):
    r = rigs(shape, precision)
    q, d = r.problem(Mp, Md), r.d
    u, o7 = r.used, r.o7
    for variant in dc.VARIANTS:
        kind = "nll" if variant in ("plain", "kl_vclip") else "mse"
        tag = (shape, precision, Mp, Md, variant, kind)
        cache = variant != "plain"                          # (the plain entry's adam = 0 form is mi_ppo_forward_backward, which has no cache)
        # demo_coef = 0: the gradient buffer and the scalars are the matching existing entry's on the PPO rows alone
        r.restore(q)
        zero = r.step(q, "flat", variant, kind, coef=0.0, adam=False, cache=cache)
        r.restore(q)
        plain = r.existing(q, variant, False, cache=cache)
        n5 = 5 + 2 * r.A
        assert bool((zero[4][u] == plain[2][u]).all()), tag
        assert bool((zero[1][:n5] == plain[1][:n5]).all()), tag
        r.restore(q)
        zero1 = r.step(q, "flat", variant, kind, coef=0.0)
        r.restore(q)
        plain1 = r.existing(q, variant, True)
        dist = max(float((x - y)[u].abs().max()) for x, y in zip(zero1[0], plain1[0]))
        print("\n%s: demo_coef = 0 against the existing entry: parameters and slots %.3e apart (%s)" %
              (tag, dist, "bitwise" if all(bitwise(x[u], y[u]) for x, y in zip(zero1[0], plain1[0])) else "not bitwise"))
        assert dist <= 1e-7, tag
        # any demo_coef: the value net's range of the gradient buffer is the plain step's
        r.restore(q)
        g = r.step(q, "flat", variant, kind, adam=False, cache=cache)
        assert bool((g[4][o7:][u[o7:]] == plain[2][o7:][u[o7:]]).all()) and not bool((g[4][:o7][u[:o7]] == plain[2][:o7][u[:o7]]).all()), tag
        assert bool((g[5][Mp:] == 0.0).all()), tag
        # two runs are bitwise equal; the row-list form is bitwise the contiguous form
        r.restore(q)
        first = r.step(q, "flat", variant, kind)
        r.restore(q)
        again = r.step(q, "flat", variant, kind)
        r.restore(q)
        gathered = r.step(q, "idx", variant, kind)
        assert all(bitwise(x, y) for x, y in zip(first, again)), tag
        assert all(bitwise(x, y) for x, y in zip(first[:4], gathered[:4])) and bitwise(first[5], gathered[5]), tag
        r.restore(q)
        g_idx = r.step(q, "idx", variant, kind, adam=False, cache=cache)
        assert bitwise(g[4][u], g_idx[4][u]), tag
        # on a recording communicator: adam = 0 followed by the optimiser
        r.restore(q)
        dp = r.step(q, "flat", variant, kind, comm=recording_comm)
        r.restore(q)
        r.step(q, "flat", variant, kind, adam=False)
        d.apply_adam(ALPHA)
        assert bitwise([d.params, d.adam_m, d.adam_v], dp[0]) and bitwise(dp[1], first[1]) and bitwise(dp[3], first[3]), tag
        if Mp + Md <= 256:                                  # the in-tile Adam against the flat one
            assert float((first[0][0] - d.params)[u].abs().max()) <= 1e-7, tag
        # with clipping by the global norm, which sees the whole gradient: "gradient buffer x factor in fp32, then mi_ppo_apply_adam"
        r.restore(q)
        d.set_max_grad_norm(0.5)
        clipped = r.step(q, "flat", variant, kind)
        rec = d.grad_clip.clone()
        assert rec[2].item() == 0.5 and 0.0 < rec[1].item() <= 1.0 and rec[0].item() > 0.0, tag
        r.restore(q)
        gfull = r.step(q, "flat", variant, kind, adam=False)[4]
        norm = float(np.sqrt(sum(float((gfull[o_:o_ + s_].double() ** 2).sum()) for _, (o_, s_) in d.layout.items())))
        assert rec[0].item() == pytest.approx(norm, rel=1e-6), tag
        d.grads.mul_(rec[1])
        d.apply_adam(ALPHA)
        assert bitwise([d.params, d.adam_m, d.adam_v], clipped[0]), tag
    r.restore(q)


def test_c_refusals_write_nothing(rigs):
    import torch
    from mi355 import lib as milib
    r = rigs("A3", "fp32")
    q, d = r.problem(33, 7), r.d
    cdll, protos = d.L.cdll, milib.parse_header()
    name = "mi_ppo_train_step_demo"
    fn = getattr(cdll, name)
    fn.restype, fn.argtypes = ctypes.c_int, [milib._CTYPES[t] for t, _ in protos[name][1]]
    watched = lambda x: (x.params, x.adam_m, x.adam_v, x.params_old, x.grads, x.losses, x.kl_losses, x.demo_losses, x.action_mean, x.value_head_grad)      # noqa: E731
    for t in (d.losses, d.kl_losses, d.demo_losses, d.action_mean, d.value_head_grad):
        t.fill_(-3.0)                                       # sentinels in every buffer a step writes
    before = [x.clone() for x in watched(d)]
    p, st, inf, nan = milib.ptr, d.stream(), float("inf"), float("nan")
    good = dict(h=d.handle, comm=None, stream=st, states=p(q.tab["s"]), actions=p(q.tab["a"]), returns=p(q.tab["R"]), advantage=p(q.tab["adv"]), logp_old=p(q.tab["lp"]),
                mean_old=p(q.tab["mo"]), kl_on=1, kl_coef=0.7, old_values=p(q.tab["vo"]), clip_range_vf=0.2, row_idx=p(q.rows), n_rows=int(q.tab["s"].shape[0]), M=33,
                demo_states=p(q.tab["ds"]), demo_actions=p(q.tab["da"]), demo_row_idx=p(q.drows), n_demo_rows=int(q.tab["ds"].shape[0]), M_demo=7, demo_kind=0,
                demo_coef=0.5, inv_m_demo=1.0 / 7, inv_m=1.0 / 33, grad_scale=1.0, adam=1, alpha=ALPHA, beta1=0.9, beta2=0.999, epsilon=1e-8)
    assert [n for _, n in protos[name][1]] == list(good)
    for change, code, text in ((dict(h=None), -4, "null handle"), (dict(M=0), -1, "batch outside"), (dict(M_demo=0), -1, "M_demo is at least 1"),
                               (dict(M=314), -1, "exceeds max_batch"), (dict(M_demo=288), -1, "exceeds max_batch"), (dict(n_rows=0), -1, "empty tables"),
                               (dict(n_demo_rows=0), -1, "are not empty"), (dict(demo_states=None), -1, "missing buffers (demo_states"),
                               (dict(demo_actions=None), -1, "missing buffers (demo_states"), (dict(states=None), -1, "missing buffers (states"),
                               (dict(demo_kind=2), -1, "demo_kind is 0"), (dict(demo_kind=-1), -1, "demo_kind is 0"), (dict(demo_coef=-0.5), -1, "demo_coef is a finite"),
                               (dict(demo_coef=nan), -1, "demo_coef is a finite"), (dict(demo_coef=inf), -1, "demo_coef is a finite"),
                               (dict(inv_m_demo=0.0), -1, "inv_m_demo is"), (dict(inv_m_demo=nan), -1, "inv_m_demo is"), (dict(inv_m_demo=-1.0), -1, "inv_m_demo is"),
                               (dict(kl_on=2), -1, "kl_on is 0"), (dict(mean_old=None), -1, "come together"), (dict(logp_old=None), -1, "come together"),
                               (dict(kl_coef=-1.0), -1, "kl_coef is a finite"), (dict(kl_coef=inf), -1, "kl_coef is a finite"),
                               (dict(clip_range_vf=0.0), -1, "clip_range_vf is a positive"), (dict(adam=2), -1, "adam is 0")):
        args = dict(good)
        args.update(change)
        rc = fn(*[args[n] for _, n in protos[name][1]])
        msg = cdll.mi_last_error().decode()
        assert rc == code and msg.startswith(name + ": ") and text in msg, (change, rc, msg)
    # an engine outside the fused range (131 inputs with wide inputs off): MI_ERR_SHAPE by name, nothing launched
    from mi355.ppo_device import PpoDevice
    low, high = bc.bounds(2)
    w = PpoDevice(131, 2, low, high, 0.2, 0.5, 0.01, max_batch=64)
    assert not w.fused_ok()
    z = lambda *s: torch.zeros(*s, device=w.device)      # noqa: E731
    w.grads.fill_(FILL)
    wb = [x.clone() for x in watched(w)]
    with pytest.raises(milib.MiError, match=name + ": needs the fused kernels"):
        w.train_step_demo(None, z(33, 131), z(33, 2), z(33), z(33), None, None, None, None, 33, z(7, 131), z(7, 2), None, 7, "nll", 0.5, 1.0 / 7, 1.0 / 33, 1.0, ALPHA)
    torch.cuda.synchronize()
    assert bitwise(wb, list(watched(w)))
    w.close()
    torch.cuda.synchronize()
    assert bitwise(before, list(watched(d)))
    r.restore(q)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the buffers: the smallest MlpVAE, 72 -> (36,) -> 8 with 3 measurements and 2 actions (tests/test_zzzzzzzzzz_behaviour_cloning_gpu.py), a demonstration buffer of 11 rows
# ---------------------------------------------------------------------------------------------------------------------------------------
MLP_SRC, MLP_ENC, MLP_Z, N_MEAS, N_DEMO = (4, 6, 3), (36,), 8, 3, 11
GAMMA, LAM = 0.99, 0.95


@pytest.fixture(scope="module")
def mlp_vae(tmp_path_factory):
    from oracle import vae_oracle as vo
    from vae.models import MlpVAE
    rng = np.random.RandomState(21)
    p = vo.init_mlp_vae_params(3, z_dim=MLP_Z, source_shape=MLP_SRC, target_shape=MLP_SRC, encoder_sizes=MLP_ENC, decoder_sizes=(8,))
    for k in p:
        if k.endswith("bias"):
            p[k] = (0.05 * rng.standard_normal(p[k].shape)).astype(np.float32)
    v = MlpVAE(np.array(MLP_SRC), encoder_sizes=MLP_ENC, decoder_sizes=(8,), z_dim=MLP_Z, model_dir=str(tmp_path_factory.mktemp("demo_vae")), precision="fp32", training=False)
    v.set_weights(p)
    v.init_session(init_logging=False)
    yield v
    v.dev.close()


def frames_and_measurements(rng, n):
    frames = rng.randint(0, 256, (n,) + MLP_SRC, dtype=np.uint8)
    meas = np.stack([rng.uniform(-1, 1, n), rng.uniform(0, 1, n), rng.uniform(0, 30, n)], axis=1)
    return frames, meas


def demonstrations(vae, m, n=N_DEMO, seed=70):
    from oracle import ppo_oracle as po
    from rollout import DemonstrationBuffer
    rng = np.random.RandomState(seed)
    db = DemonstrationBuffer(vae, m, 16, chunk=8, seed=3)
    if n:
        frames, meas = frames_and_measurements(rng, n)
        space = po.ActionSpace()
        db.add(frames, meas, rng.uniform(space.low, space.high, (n, len(space.low))).astype(np.float32))
    return db


def collected(cls, vae, m, E, T, seed=81):
    """A buffer of class cls with a collection in it: lane 1 reports done at its step 3, the others run the horizon out."""
    buf = cls(vae, m, E, T, seed=3)
    collect(buf, E, T, seed)
    return buf


def collect(buf, E, T, seed=81):
    from rollout import ContinuousRolloutBuffer
    rng = np.random.RandomState(seed)
    buf.reset()
    if isinstance(buf, ContinuousRolloutBuffer):
        for t in range(1, T + 1):
            f, ms = frames_and_measurements(rng, E)
            buf.step(f, ms, noise=rng.standard_normal((E, 2)).astype(np.float32))
            buf.outcome(rng.uniform(0, 1, E), np.array([e == 1 and t == 3 for e in range(E)]))
        need = buf.rows.needs_bootstrap()
        f, ms = frames_and_measurements(rng, E)
        buf.bootstrap(f[need], ms[need], env_ids=need)
    else:
        live, t = np.arange(E), 0
        while len(live):
            f, ms = frames_and_measurements(rng, len(live))
            buf.step(f, ms, env_ids=live, noise=rng.standard_normal((len(live), 2)).astype(np.float32))
            dones = np.array([int(e) == 1 and t + 1 == 3 for e in live])
            buf.outcome(rng.uniform(0, 1, len(live)), dones, env_ids=live)
            t += 1
            live = live[~dones & (buf.lengths[live] < T)]
        f, ms = frames_and_measurements(rng, E)
        buf.bootstrap(f, ms)


def buffer_cases():
    from rollout import ContinuousRolloutBuffer, RolloutBuffer
    return [(RolloutBuffer, 3, 5, 4, False), (ContinuousRolloutBuffer, 3, 5, 32, False), (RolloutBuffer, 5, 20, 32, True), (ContinuousRolloutBuffer, 5, 20, 4, True)]


@pytest.mark.parametrize("case", range(4))
def test_update_is_a_host_loop_of_demo_steps(mlp_vae, tmp_path, case):
    """update() with the setting on against PpoDevice.train_step_demo over the same PPO permutation and the restated draw rule on a twin policy, bitwise; the legacy
    numpy stream ends where the same update with the setting off leaves it; set_demonstrations(None) is bitwise a buffer that never had the setting.  The (5, 20)
    cases run with value clipping and the KL penalty on."""
    import torch
    from ppo import ADAM_BETA1, ADAM_BETA2, _adam_alpha
    cls, E, T, demo_bs, settings = buffer_cases()[case]
    din, batch, epochs, coef, decay = MLP_Z + N_MEAS, 8, 2, 0.6, 0.5
    pols = [make_pair(tmp_path / n, input_dim=din)[1] for n in ("m", "twin", "off", "never")]
    m, twin, off, never = pols
    if settings:
        for x in pols:
            x.set_value_clip(0.2)
            x.set_kl_penalty(0.7)
    assert all(bitwise(flat_state(m), flat_state(x)) for x in pols[1:])
    db = demonstrations(mlp_vae, m)
    buf = collected(cls, mlp_vae, m, E, T)
    buf.set_demonstrations(db, coef, loss="nll" if case % 2 == 0 else "mse", batch_size=demo_bs, decay=decay, seed=7)
    kind = "nll" if case % 2 == 0 else "mse"
    np.random.seed(11)
    out = buf.update(GAMMA, LAM, num_epochs=epochs, batch_size=batch)
    rng_after = np.random.get_state()
    valid = buf.rows.valid_rows()
    n_valid, md = len(valid), min(demo_bs, N_DEMO)
    steps = epochs * -(-n_valid // batch)
    assert len(out["losses"]) == steps == len(out["demo_losses"]) == len(out["demo_rows"]) and set(out["demo_losses"][0]) == {"demo_loss", "mean_sq_error"}
    assert out["demo_coef"] == coef and out["demo_coef_next"] == coef * decay
    # the demonstration rows of every step: the stated draw rule
    want_rows = dc.demonstration_rows(np.random.RandomState(7), [None, 0], N_DEMO, demo_bs, steps)
    assert all(np.array_equal(a, b) for a, b in zip(out["demo_rows"], want_rows)) and all(len(a) == md for a in out["demo_rows"])
    # the host loop on the twin: the tables of the buffer (theta_old of both policies is the same theta), the same device calls
    twin.update_old_policy()
    np.random.seed(11)
    k, want, want_demo = 0, [], []
    for _ in range(epochs):
        idx = np.arange(n_valid)
        np.random.shuffle(idx)
        perm = torch.from_numpy(valid[idx]).to(buf.device)
        for i in range(0, n_valid, batch):
            mb = perm[i:i + batch]
            n = int(mb.numel())
            alpha = _adam_alpha(twin.current_learning_rate(), twin.beta1_power, twin.beta2_power)
            twin.dev.train_step_demo(None, buf.states, buf.actions, buf.returns, buf.advantages, buf.logp_old, buf.mean_old if settings else None,
                                     0.7 if settings else None, mb, n, db.states, db.expert_actions, torch.from_numpy(want_rows[k]).to(buf.device), md, kind, coef,
                                     1.0 / md, 1.0 / n, 1.0, alpha, old_values=buf.values if settings else None, clip_range_vf=0.2 if settings else None)
            twin.beta1_power, twin.beta2_power = np.float32(twin.beta1_power * np.float32(ADAM_BETA1)), np.float32(twin.beta2_power * np.float32(ADAM_BETA2))
            want.append(twin.dev.losses[:5].cpu().numpy())
            D = twin.dev.demo_losses.cpu().numpy()
            want_demo.append({"demo_loss": float(D[0]), "mean_sq_error": float(D[2])})
            k += 1
    assert bitwise(flat_state(m), flat_state(twin)) and m.beta1_power == twin.beta1_power and m.train_step_counter == steps
    keys = ("policy_loss", "value_loss", "entropy_loss", "loss", "prob_ratio")
    assert [[rec[x] for x in keys] for rec in out["losses"]] == [[float(v) for v in row] for row in want]
    assert out["demo_losses"] == want_demo
    assert all(rec["demo_loss"] > 0 for rec in out["demo_losses"])
    if settings:
        assert "kl" in out and len(out["losses"][0]) == 7
    # the setting switched off again, and a buffer that never had it: bitwise each other, no key of the setting, and the numpy stream where the update above left it
    results = []
    for x, touch in ((off, True), (never, False)):
        b = collected(cls, mlp_vae, x, E, T)
        if touch:
            b.set_demonstrations(demonstrations(mlp_vae, x), coef, batch_size=demo_bs)
            b.set_demonstrations(None)
        np.random.seed(11)
        results.append(b.update(GAMMA, LAM, num_epochs=epochs, batch_size=batch))
        state = np.random.get_state()
        assert state[0] == rng_after[0] and np.array_equal(state[1], rng_after[1]) and state[2:] == rng_after[2:]
        assert not [key for key in results[-1] if key.startswith("demo")]
    assert bitwise(flat_state(off), flat_state(never)) and results[0]["losses"] == results[1]["losses"]
    assert not bitwise(flat_state(m), flat_state(never))
    for x in pols:
        x.dev.close()


def test_decay_state_round_trip_and_refusals(mlp_vae, tmp_path, monkeypatch):
    import torch
    from rollout import ContinuousRolloutBuffer, RolloutBuffer
    din, E, T = MLP_Z + N_MEAS, 3, 5
    _, m = make_pair(tmp_path / "m", input_dim=din)
    _, other = make_pair(tmp_path / "o", input_dim=din)
    db = demonstrations(mlp_vae, m)
    buf = collected(ContinuousRolloutBuffer, mlp_vae, m, E, T)
    with pytest.raises(ValueError, match="the demonstration term is off"):
        buf.demonstration_state()
    buf.set_demonstrations(db, 0.8, batch_size=4, decay=0.5, seed=5)
    np.random.seed(3)
    a = buf.update(GAMMA, LAM, num_epochs=1, batch_size=8)
    assert (a["demo_coef"], a["demo_coef_next"]) == (0.8, 0.4)
    saved = buf.demonstration_state()
    assert saved["coef"] == 0.4 and saved["cursor"] == 8 and sorted(saved["perm"].tolist()) == list(range(N_DEMO))
    collect(buf, E, T, seed=82)
    np.random.seed(4)
    b = buf.update(GAMMA, LAM, num_epochs=1, batch_size=8)
    assert (b["demo_coef"], b["demo_coef_next"]) == (0.4, 0.2)
    # a second buffer that loads the saved state draws the same rows with the same coefficient
    buf2 = ContinuousRolloutBuffer(mlp_vae, m, E, T, seed=3)
    buf2.set_demonstrations(db, 0.123, batch_size=4, decay=0.5, seed=99)
    buf2.load_demonstration_state(saved)
    collect(buf2, E, T, seed=82)
    np.random.seed(4)
    c = buf2.update(GAMMA, LAM, num_epochs=1, batch_size=8)
    assert c["demo_coef"] == 0.4 and all(np.array_equal(x, y) for x, y in zip(b["demo_rows"], c["demo_rows"]))
    again = buf2.demonstration_state()
    now = buf.demonstration_state()
    assert again["coef"] == now["coef"] and again["cursor"] == now["cursor"] and np.array_equal(again["perm"], now["perm"]) and np.array_equal(again["rng"][1], now["rng"][1])
    for bad in ({}, dict(saved, coef=-1.0), dict(saved, cursor=99), dict(saved, perm=[0, 0, 1]), dict(saved, rng=("x",))):
        with pytest.raises(ValueError, match="load_demonstration_state"):
            buf2.load_demonstration_state(bad)
    # refusals, before anything is launched
    fresh = RolloutBuffer(mlp_vae, m, E, T, seed=3)
    for kw, text in ((dict(coef=-1.0), "coef is a finite"), (dict(coef=float("nan")), "coef is a finite"), (dict(coef=True), "coef is a finite"),
                     (dict(coef=0.5, loss="huber"), 'the loss is "nll"'), (dict(coef=0.5, batch_size=0), "batch_size is an int"),
                     (dict(coef=0.5, decay=float("inf")), "decay is a finite"), (dict(coef=0.5, seed=-1), "seed is an int")):
        with pytest.raises(ValueError, match=text):
            fresh.set_demonstrations(db, **kw)
    with pytest.raises(ValueError, match="DemonstrationBuffer or None"):
        fresh.set_demonstrations(buf, 0.5)
    with pytest.raises(ValueError, match="the demonstration buffer is empty"):
        fresh.set_demonstrations(demonstrations(mlp_vae, m, n=0), 0.5)
    with pytest.raises(ValueError, match="another ppo object"):
        fresh.set_demonstrations(demonstrations(mlp_vae, other), 0.5)
    narrow = demonstrations(mlp_vae, m)
    narrow.states = torch.zeros(16, din + 1, device=narrow.device)
    with pytest.raises(ValueError, match="the demonstration buffer's rows are"):
        fresh.set_demonstrations(narrow, 0.5)
    narrow = demonstrations(mlp_vae, m)
    narrow.A = 3
    with pytest.raises(ValueError, match="the demonstration buffer's rows are"):
        fresh.set_demonstrations(narrow, 0.5)
    _, m19 = make_pair(tmp_path / "s", input_dim=2 * MLP_Z + N_MEAS)
    with pytest.raises(ValueError, match="latent stacking is on"):
        RolloutBuffer.stacked(mlp_vae, m19, E, T, 2, seed=3).set_demonstrations(db, 0.5)
    # observation normalisation: off in both, or frozen here and equal to the state the demonstration buffer was given
    fresh.set_observation_normalization()
    with pytest.raises(ValueError, match="on in one buffer and off in the other"):
        fresh.set_demonstrations(db, 0.5)
    normed = demonstrations(mlp_vae, m, n=0)
    normed.set_observation_normalization(fresh.observation_normalization_state())
    frames, meas = frames_and_measurements(np.random.RandomState(1), 3)
    normed.add(frames, meas, np.zeros((3, 2), np.float32))
    with pytest.raises(ValueError, match="must be frozen and equal"):
        fresh.set_demonstrations(normed, 0.5)               # (not frozen here)
    fresh.set_observation_normalization(frozen=True)
    fresh.set_demonstrations(normed, 0.5)
    fresh.set_observation_normalization(frozen=True, clip=5.0)
    with pytest.raises(ValueError, match="must be frozen and equal"):
        fresh.set_demonstrations(normed, 0.5)
    fresh.set_observation_normalization(None)
    fresh.set_demonstrations(None)
    with pytest.raises(ValueError, match="on in one buffer and off in the other"):
        fresh.set_demonstrations(normed, 0.5)
    # a buffer emptied behind the setting is refused by update(), and a policy outside the fused range (here: the fused kernels switched off) by both
    fresh.set_demonstrations(db, 0.5)
    collect(fresh, E, T)
    db.reset()
    with pytest.raises(ValueError, match="update: the demonstration buffer is empty"):
        fresh.update(GAMMA, LAM, num_epochs=1, batch_size=8)
    full = demonstrations(mlp_vae, m)
    monkeypatch.setenv("MI355_PPO_FUSED", "0")
    with pytest.raises(ValueError, match="exists only in the fused kernels"):
        fresh.set_demonstrations(full, 0.5)
    monkeypatch.delenv("MI355_PPO_FUSED")
    with pytest.raises(ValueError, match="PPO._demo_rows: the demonstration term is off"):
        other._demo_rows(*[None] * 14)
    for x in (m, other, m19):
        x.dev.close()
