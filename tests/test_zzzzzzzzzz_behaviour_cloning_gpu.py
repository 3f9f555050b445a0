"""Behaviour cloning on the GPU: mi_ppo_clone_step through PpoDevice.clone_step / PPO.clone_step, and rollout.DemonstrationBuffer.

Engines, sizes, inputs, the float64 reference (numpy alone) and the bounds: tests/behaviour_cloning_cases.py.  Every size runs as contiguous tensors and through
row_idx into tables of 2 M + 3 rows that hold NaN in every row the index does not name; both kinds, with and without returns, fp32 and bf16x3.  Bounds: clone_loss
1e-4 of the sum of its absolute terms ("mse": 1e-4 relative), value_loss 1e-4 relative, gradients 2e-4 of each tensor's max (bf16x3: max(1e-3, 4 x the fp32
reference's own distance from float64)), parameters within 2e-6 of TF-Adam on the device's gradients where |g| > 1e-3 of the tensor's max.  Every engine starts
from NON-ZERO Adam slots, so that an Adam launch over a zero gradient would show in the value net."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import behaviour_cloning_cases as bc  # noqa: E402
from rollout_gpu_common import bitwise  # noqa: E402

ALPHA = 1e-4
FILL = 4.25
X3_GRAD_FLOOR, X3_GRAD_FACTOR = 1e-3, 4.0                # tests/test_j_ppo_bf16x3_gpu.py
GRID = [(s, p, M) for s in ("A2", "A3") for p in ("fp32", "bf16x3") for M in bc.MS]
FORMS = [(k, wr) for k in bc.KINDS for wr in (True, False)]


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


class Problem:
    pass


class Rig:
    """One engine per (shape, precision) and its problems per M: contiguous tensors and the same samples as shuffled rows of NaN-filled tables."""

    def __init__(self, shape, precision):
        import torch
        from mi355.ppo_device import PpoDevice
        self.shape, self.precision = shape, precision
        self.din, self.A, self.hidden, _ = bc.SHAPES[shape]
        low, high = bc.bounds(self.A)
        self.d = PpoDevice(self.din, self.A, low, high, 0.2, bc.VALUE_SCALE, 0.01, hidden=self.hidden, max_batch=320, precision=precision,
                           wide_inputs=1 if self.din > 96 else 0)
        assert self.d.fused_ok()
        self.o7 = self.d.layout[bc.NAMES[7]][0]            # where the value net starts in the flat buffers
        self.used = torch.zeros(self.d.n_flat, dtype=torch.bool, device=self.d.device)
        for _, (o_, s_) in self.d.layout.items():
            self.used[o_:o_ + s_] = True
        self.problems = {}

    def restore(self, q, fill=FILL):
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
        q.M, q.c = M, bc.case(self.shape, M)
        c = q.c
        rng = np.random.RandomState(500 + M)
        d.load_params(c.theta, {k.replace("policy/", "policy_old/", 1): v for k, v in c.theta.items()})
        q.m0 = {k: (0.01 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in c.theta.items()}
        q.v0 = {k: ((0.01 * rng.standard_normal(v.shape)) ** 2 + 1e-6).astype(np.float32) for k, v in c.theta.items()}
        d.load_slots(q.m0, q.v0)
        q.state0, q.old = [x.clone() for x in (d.params, d.adam_m, d.adam_v)], d.params_old.clone()
        q.s, q.a, q.R = self.up(c.s), self.up(c.a), self.up(c.R)
        n = 2 * M + 3
        rows = rng.permutation(n)[:M].astype(np.int32)
        q.rows = torch.from_numpy(rows).to(d.device)
        idx = q.rows.long()
        q.tab = {}
        for name, x, width in (("s", q.s, self.din), ("a", q.a, A), ("R", q.R, 0)):
            t = torch.full((n, width) if width else (n,), float("nan"), device=d.device)
            t[idx] = x
            q.tab[name] = t
        self.problems[M] = q
        self.restore(q)
        return q

    def step(self, q, form, kind, with_returns, adam=True, comm=None):
        """One clone step from the state the engine is in -> (params / m / v, the five loss floats, gradient buffer)."""
        d, M = self.d, q.M
        flat = form == "flat"
        s, a, R = (q.s, q.a, q.R) if flat else (q.tab["s"], q.tab["a"], q.tab["R"])
        d.clone_step(comm, s, a, R if with_returns else None, kind, None if flat else q.rows, M, 1.0 / M, 1.0, ALPHA, adam=adam)
        return [x.clone() for x in (d.params, d.adam_m, d.adam_v)], d.losses[:5].clone(), d.grads.clone()


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


def check_against_float64(r, q, form, kind, wr):
    import torch
    d, tag = r.d, (r.shape, r.precision, q.M, form, kind, wr)
    scal, g64, _, _ = bc.reference(r.shape, q.M, kind, wr)
    g32 = bc.reference(r.shape, q.M, kind, wr, dtype=np.float32)[1]
    r.restore(q)
    state, losses, gbuf = r.step(q, form, kind, wr, adam=False)
    g, L = d.export_grads(), losses.cpu().numpy()
    names = bc.NAMES if wr else bc.POLICY_NET
    floor = scal["abs_terms"] if kind == "nll" else scal["clone_loss"]
    print("\n%s: clone_loss %.9g (float64 %.9g, error %.2e of the absolute terms), value_loss %.9g (%.9g), mean_sq_error %.9g (%.9g)" %
          (tag, L[0], scal["clone_loss"], abs(L[0] - scal["clone_loss"]) / floor, L[1], scal["value_loss"], L[4], scal["mean_sq_error"]))
    assert abs(float(L[0]) - scal["clone_loss"]) <= bc.LOSS_REL * floor, tag
    if wr:
        assert float(L[1]) == pytest.approx(scal["value_loss"], rel=bc.LOSS_REL), tag
    else:
        assert L[1] == 0.0, tag
    assert L[2] == 0.0 and abs(float(L[3]) - scal["loss"]) <= bc.LOSS_REL * (floor + scal["value_loss"]), tag
    assert L[3].tobytes() == (L[0] + L[1]).astype(np.float32).tobytes(), tag
    assert float(L[4]) == pytest.approx(scal["mean_sq_error"], rel=bc.LOSS_REL), tag
    bound = {k: bc.GRAD_REL if r.precision == "fp32" else max(X3_GRAD_FLOOR, X3_GRAD_FACTOR * rel_err(g32[k], g64[k])) for k in names}
    if kind == "mse":                                       # exactly zero in the reference and on the device
        assert not g[bc.NAMES[6]].any() and not g64[bc.NAMES[6]].any(), tag
        names = [k for k in names if k != bc.NAMES[6]]
    err = {k: rel_err(g[k], g64[k]) for k in names}
    for k in names:
        print("  %-28s %.3e of max (bound %.1e)" % (k, err[k], bound[k]))
    assert not {k: (err[k], bound[k]) for k in names if err[k] > bound[k]}, tag
    assert bitwise(state, q.state0), tag                    # adam = 0 leaves the parameters and the optimiser state alone
    if not wr:                                              # policy only: the value net's range of the gradient buffer is exactly 0.0
        assert bool((gbuf[r.o7:] == 0.0).all()) and not bool(torch.signbit(gbuf[r.o7:]).any()), tag
    assert bool((gbuf[:r.o7][r.used[:r.o7]] != FILL).all()), tag
    # adam = 1: TF-Adam on the device's own gradients, from the non-zero slots
    r.restore(q)
    after = r.step(q, form, kind, wr, adam=True)
    p1 = d.export_params()
    for k in names:
        want, _, _ = bc.adam_tf(q.c.theta[k], q.m0[k], q.v0[k], g[k], np.float32(ALPHA))
        big = np.abs(g[k]) > bc.ADAM_GMIN * np.abs(g[k]).max()
        assert big.any() and np.abs(p1[k].astype(np.float64) - want)[big].max() <= bc.ADAM_ABS, (tag, k, float(np.abs(p1[k] - want)[big].max()))
    assert not bitwise(after[0][0], q.state0[0]), tag
    if not wr:                                              # ... and the value net's parameters and both slots keep their bits
        for x, y in zip(after[0], q.state0):
            assert bitwise(x[r.o7:], y[r.o7:]), tag
    r.restore(q)


@pytest.mark.parametrize("form", ["flat", "idx"])
@pytest.mark.parametrize("shape,precision,M", GRID)
def test_clone_step_against_float64(rigs, shape, precision, M, form):
    r = rigs(shape, precision)
    q = r.problem(M)
    for kind, wr in FORMS:
        check_against_float64(r, q, form, kind, wr)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_wide_inputs_against_float64(rigs, precision):
    r = rigs("W", precision)
    assert r.d.engine_wide_inputs() == 1 and r.d.kin > 96
    q = r.problem(33)
    for form in ("flat", "idx"):
        for kind, wr in FORMS:
            check_against_float64(r, q, form, kind, wr)


@pytest.mark.parametrize("shape,precision,M", [g for g in GRID if g[2] != 5])
def test_identities(rigs, recording_comm, shape, precision, M):
    import torch
    r = rigs(shape, precision)
    q, d = r.problem(M), r.d
    for kind, wr in FORMS:
        tag = (shape, precision, M, kind, wr)
        # two runs are bitwise equal; the row_idx form is the contiguous form on the gathered rows
        r.restore(q)
        first = r.step(q, "flat", kind, wr)
        r.restore(q)
        again = r.step(q, "flat", kind, wr)
        r.restore(q)
        gathered = r.step(q, "idx", kind, wr)
        assert all(bitwise(x, y) for x, y in zip(first, again)), tag
        assert all(bitwise(x, y) for x, y in zip(first[:2], gathered[:2])), tag
        r.restore(q)
        g_flat = r.step(q, "flat", kind, wr, adam=False)[2]
        r.restore(q)
        g_idx = r.step(q, "idx", kind, wr, adam=False)[2]
        assert bitwise(g_flat[r.used], g_idx[r.used]), tag
        if wr:
            # the six value-net gradients are those of mi_ppo_forward_backward on the same states and returns
            r.restore(q)
            d.forward_backward(q.s, q.a, q.R, torch.zeros(M, device=d.device), M, 1.0 / M, 1.0)
            assert bitwise(d.grads[r.o7:][r.used[r.o7:]], g_flat[r.o7:][r.used[r.o7:]]), tag
        # on a recording communicator: adam = 0 followed by the optimiser (policy only: over the policy's prefix, so the value net keeps its bits)
        r.restore(q)
        dp = r.step(q, "flat", kind, wr, comm=recording_comm)
        if wr:
            r.restore(q)
            r.step(q, "flat", kind, wr, adam=False)
            d.apply_adam(ALPHA)
            assert bitwise([d.params, d.adam_m, d.adam_v], dp[0]) and bitwise(dp[1], first[1]), tag
            if M <= 256:                                    # the in-tile Adam against the flat one
                assert float((first[0][0] - d.params)[r.used].abs().max()) <= 1e-7, tag      # (the alignment gaps hold the test's fill: only the flat Adam sees them)
        else:
            for x, y in zip(dp[0], q.state0):
                assert bitwise(x[r.o7:], y[r.o7:]), tag
            assert float((first[0][0] - dp[0][0])[r.used].abs().max()) <= 1e-7 and not bitwise(dp[0][0][:r.o7], q.state0[0][:r.o7]), tag
        # with clipping by the global norm: "gradient buffer x factor in fp32, then mi_ppo_apply_adam"
        r.restore(q)
        d.set_max_grad_norm(0.5)
        clipped = r.step(q, "flat", kind, wr)
        rec = d.grad_clip.clone()
        assert rec[2].item() == 0.5 and 0.0 < rec[1].item() <= 1.0 and rec[0].item() > 0.0, tag
        if wr:
            r.restore(q)
            r.step(q, "flat", kind, wr, adam=False)
            d.grads.mul_(rec[1])
            d.apply_adam(ALPHA)
            assert bitwise([d.params, d.adam_m, d.adam_v], clipped[0]), tag
        else:
            for x, y in zip(clipped[0], q.state0):
                assert bitwise(x[r.o7:], y[r.o7:]), tag
            assert not bitwise(clipped[0][0][:r.o7], q.state0[0][:r.o7]), tag
    r.restore(q)


@pytest.mark.parametrize("kind,wr", FORMS)
def test_16_chained_steps_follow_the_float64_trajectory(rigs, kind, wr):
    """16 steps at M = 33 from zero slots: per tensor no further from the float64 trajectory than 2 x the reference's fp32 twin + 2e-4 of the update, all three as
    RMS over the tensor's entries -- the norm tests/test_zz_adam_trajectory_gpu.py states the same sentence in, for its reason: Adam's first steps move every entry
    by ~lr whatever its gradient's size, so the last bit of a ~zero gradient entry decides that entry's direction, in the fp32 twin as much as on the device, and
    the LARGEST entry error of a tensor is the luck of which entries sit there.  (The first form of this test took the maximum: the policy net passed, and
    policy/dense_2/kernel -- the value net, whose arithmetic is bitwise mi_ppo_forward_backward's -- measured 6.9e-6 against the twin's 6.4e-7 and a bound of
    4.2e-6.)  The maxima are printed beside the RMS figures."""
    r = rigs("A2", "fp32")
    q, d, c = r.problem(33), r.d, bc.case("A2", 33)
    d.adam_m.zero_()
    d.adam_v.zero_()
    for t in range(1, 17):
        d.clone_step(None, q.s, q.a, q.R if wr else None, kind, None, 33, 1.0 / 33, 1.0, bc.adam_alpha(bc.LR, t, np.float32))
    got = d.export_params()
    t64, t32 = bc.trajectory(c, kind, wr, 16), bc.trajectory(c, kind, wr, 16, dtype=np.float32)
    for k in (bc.NAMES if wr else bc.POLICY_NET):
        if kind == "mse" and k == bc.NAMES[6]:
            assert np.array_equal(got[k], c.theta[k])       # a gradient of exactly 0 from zero slots moves nothing
            continue
        rms = lambda x: float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))      # noqa: E731
        update, dist, twin = rms(t64[k] - c.theta[k]), rms(got[k] - t64[k]), rms(t32[k] - t64[k])
        print("%-28s RMS: device %.3e, fp32 twin %.3e, update %.3e;  max: device %.3e, fp32 twin %.3e, update %.3e" %
              (k, dist, twin, update, np.abs(got[k] - t64[k]).max(), np.abs(t32[k] - t64[k]).max(), np.abs(t64[k] - c.theta[k]).max()))
        assert update > 0 and dist <= 2 * twin + 2e-4 * update, (k, dist, twin, update)
    r.restore(q)


def test_c_refusals_write_nothing(rigs):
    import torch
    from mi355 import lib as milib
    r = rigs("A3", "fp32")
    q, d = r.problem(33), r.d
    cdll, protos = d.L.cdll, milib.parse_header()
    fn = cdll.mi_ppo_clone_step
    fn.restype, fn.argtypes = ctypes.c_int, [milib._CTYPES[t] for t, _ in protos["mi_ppo_clone_step"][1]]
    d.losses.fill_(-3.0)
    before = [x.clone() for x in (d.params, d.adam_m, d.adam_v, d.params_old, d.grads, d.losses)]
    p, st = milib.ptr, d.stream()
    good = dict(h=d.handle, comm=None, stream=st, states=p(q.tab["s"]), expert_actions=p(q.tab["a"]), returns=p(q.tab["R"]), kind=0, row_idx=p(q.rows),
                n_rows=int(q.tab["s"].shape[0]), M=33, inv_m=1.0 / 33, grad_scale=1.0, adam=1, alpha=ALPHA, beta1=0.9, beta2=0.999, epsilon=1e-8)
    for change, code, text in ((dict(h=None), -4, "null handle"), (dict(M=0), -1, "batch outside"), (dict(M=321), -1, "batch outside"), (dict(kind=2), -1, "kind is 0"),
                               (dict(kind=-1), -1, "kind is 0"), (dict(n_rows=0), -1, "empty tables"), (dict(adam=2), -1, "adam is 0"),
                               (dict(states=None), -1, "missing buffers"), (dict(expert_actions=None), -1, "missing buffers")):
        args = dict(good)
        args.update(change)
        rc = fn(*[args[n] for _, n in protos["mi_ppo_clone_step"][1]])
        msg = cdll.mi_last_error().decode()
        assert rc == code and msg.startswith("mi_ppo_clone_step: ") and text in msg, (change, rc, msg)
    # an engine without optimiser buffers, and one outside the fused range (131 inputs with wide inputs off): by name, nothing launched
    from mi355.ppo_device import PpoDevice
    low, high = bc.bounds(2)
    w = PpoDevice(131, 2, low, high, 0.2, 0.5, 0.01, max_batch=64)
    assert not w.fused_ok()
    ws, wa = torch.zeros(33, 131, device=w.device), torch.zeros(33, 2, device=w.device)
    w.grads.fill_(FILL)
    wb = [x.clone() for x in (w.params, w.adam_m, w.adam_v, w.grads)]
    with pytest.raises(milib.MiError, match="mi_ppo_clone_step: needs the fused kernels"):
        w.clone_step(None, ws, wa, None, "nll", None, 33, 1.0 / 33, 1.0, ALPHA)
    torch.cuda.synchronize()
    assert bitwise(wb, [w.params, w.adam_m, w.adam_v, w.grads])
    w.close()
    torch.cuda.synchronize()
    assert bitwise(before, [d.params, d.adam_m, d.adam_v, d.params_old, d.grads, d.losses])
    r.restore(q)


def test_ppo_clone_step_is_one_step_from_host_arrays(tmp_path):
    """PPO.clone_step against the reference: the losses it returns, Adam's powers and train_step_counter advance, learning_rate None is current_learning_rate()."""
    from oracle import ppo_oracle as po
    from ppo import PPO
    space = po.ActionSpace()
    m = PPO(np.array([67]), space, learning_rate=1e-3, lr_decay=1.0, value_scale=bc.VALUE_SCALE, model_dir=str(tmp_path), seed=3)
    m.init_session(init_logging=False)
    rng = np.random.RandomState(9)
    s = (0.5 * rng.standard_normal((33, 67))).astype(np.float32)
    a = rng.uniform(space.low, space.high, (33, 2)).astype(np.float32)
    R = rng.standard_normal(33).astype(np.float32)
    theta = m.dev.export_params()
    p0, b1 = m.dev.params.clone(), np.float32(0.9)
    for i, (kind, wr) in enumerate(FORMS):
        th = m.dev.export_params()
        scal, _, _, _ = bc.loss_and_grads(th, s, a, R if wr else None, kind, space.low, space.high, value_scale=bc.VALUE_SCALE)
        out = m.clone_step(s, a, R if wr else None, loss=kind)
        assert set(out) == {"clone_loss", "value_loss", "loss", "mean_sq_error"}
        assert abs(out["clone_loss"] - scal["clone_loss"]) <= bc.LOSS_REL * (scal["abs_terms"] if kind == "nll" else scal["clone_loss"])
        assert out["value_loss"] == pytest.approx(scal["value_loss"], rel=bc.LOSS_REL) and out["mean_sq_error"] == pytest.approx(scal["mean_sq_error"], rel=bc.LOSS_REL)
        b1 = np.float32(b1 * np.float32(0.9))
        assert m.train_step_counter == i + 1 and m.beta1_power == b1
    assert not bitwise(p0, m.dev.params) and set(theta) == set(bc.NAMES)
    # training goes on from there: the clip step still runs and advances the same counters
    m.update_old_policy()
    m.train(s, a, R, rng.standard_normal(33).astype(np.float32))
    assert m.train_step_counter == len(FORMS) + 1
    m.dev.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# DemonstrationBuffer: capacity 20 on the MlpVAE 72 -> (36,) -> 8 with 3 measurements and 2 actions, rows added as 7 + 13 with chunk = 8
# ---------------------------------------------------------------------------------------------------------------------------------------
SENT = -777.0
MLP_SRC, MLP_ENC, MLP_Z, N_MEAS = (4, 6, 3), (36,), 8, 3
CAP = 20


@pytest.fixture(scope="module")
def mlp_vae(tmp_path_factory):
    from oracle import vae_oracle as vo
    from vae.models import MlpVAE
    rng = np.random.RandomState(21)
    p = vo.init_mlp_vae_params(3, z_dim=MLP_Z, source_shape=MLP_SRC, target_shape=MLP_SRC, encoder_sizes=MLP_ENC, decoder_sizes=(8,))
    for k in p:
        if k.endswith("bias"):
            p[k] = (0.05 * rng.standard_normal(p[k].shape)).astype(np.float32)
    v = MlpVAE(np.array(MLP_SRC), encoder_sizes=MLP_ENC, decoder_sizes=(8,), z_dim=MLP_Z, model_dir=str(tmp_path_factory.mktemp("bc_vae")), precision="fp32", training=False)
    v.set_weights(p)
    v.init_session(init_logging=False)
    yield v
    v.dev.close()


def demo_inputs(seed, n, src, space):
    rng = np.random.RandomState(seed)
    frames = rng.randint(0, 256, (n,) + tuple(src), dtype=np.uint8)
    meas = np.stack([rng.uniform(-1, 1, n), rng.uniform(0, 1, n), rng.uniform(0, 30, n)], axis=1)
    expert = rng.uniform(space.low, space.high, (n, len(space.low))).astype(np.float32)
    returns = rng.standard_normal(n).astype(np.float32)
    return frames, meas, expert, returns


def guarded(buf):
    """Every table the buffer writes becomes a view of a larger tensor with 8 sentinel floats behind it."""
    import torch
    big = {}
    for name in ("states", "policy_actions", "policy_values", "expert_actions", "returns") + (("raw_states",) if buf.raw_states is not None else ()):
        t = getattr(buf, name)
        b = torch.full((t.numel() + 8,), SENT, device=t.device)
        setattr(buf, name, b[:t.numel()].view(t.shape))
        big[name] = b
    return big


def recorded(buf):
    """Wraps the buffer's step so that what every device call returned is kept."""
    kept, record = [], buf._step.record

    def wrapper(*a, **kw):
        out = record(*a, **kw)
        kept.append(out)
        return out
    buf._step.record = wrapper
    return kept


def filled(vae, m, with_returns, src=MLP_SRC, seed=70, chunk=8, capacity=CAP, parts=(7, 13)):
    from oracle import ppo_oracle as po
    from rollout import DemonstrationBuffer
    buf = DemonstrationBuffer(vae, m, capacity, chunk=chunk, seed=3)
    big, kept = guarded(buf), recorded(buf)
    frames, meas, expert, returns = demo_inputs(seed, sum(parts), src, po.ActionSpace())
    lo = 0
    for n in parts:
        rows = buf.add(frames[lo:lo + n], meas[lo:lo + n], expert[lo:lo + n], returns[lo:lo + n] if with_returns else None)
        assert np.array_equal(rows, np.arange(lo, lo + n))
        lo += n
    return buf, big, kept, (frames, meas, expert, returns)


def test_buffer_tables(mlp_vae, tmp_path):
    from rollout import BatchedRolloutStep
    from rollout_gpu_common import make_pair
    _, m = make_pair(tmp_path / "m", input_dim=MLP_Z + N_MEAS)
    buf, big, kept, (frames, meas, expert, returns) = filled(mlp_vae, m, True)
    assert buf.size == CAP and buf.has_returns is True
    assert [len(k[1]) for k in kept] == [7, 8, 5]                                    # 7, then 13 as 8 + 5: chunks of at most 8
    a = np.concatenate([k[0] for k in kept])
    v = np.concatenate([k[1] for k in kept])
    s = np.concatenate([k[2] for k in kept])
    # bitwise what the step class returned for those frames, the expert's actions and the returns bitwise what was passed
    assert np.array_equal(buf.states.cpu().numpy(), s.astype(np.float32)) and np.array_equal(s[:, MLP_Z:], meas)
    assert np.array_equal(buf.policy_actions.cpu().numpy(), a) and np.array_equal(buf.policy_values.cpu().numpy(), v)
    assert np.array_equal(buf.expert_actions.cpu().numpy().view(np.int32), expert.view(np.int32))
    assert np.array_equal(buf.returns.cpu().numpy().view(np.int32), returns.view(np.int32))
    for name, b in big.items():
        assert bool((b[-8:] == SENT).all()), name
    # a step of its own gives the same rows (to 1e-5: the encoder's split-K sums are fp32 atomics), and the call was greedy
    step = BatchedRolloutStep(mlp_vae, m, 8, seed=5)
    a2, v2, s2 = step(frames[:8], meas[:8], greedy=True)
    assert np.allclose(s2, s[:8], rtol=1e-5, atol=1e-5) and np.allclose(a2, a[:8], rtol=1e-5, atol=1e-5)
    # reset() empties the buffer and lets returns be decided anew
    buf.reset()
    assert buf.size == 0 and buf.has_returns is None
    assert np.array_equal(buf.add(frames[:3], meas[:3], expert[:3]), np.arange(3)) and buf.has_returns is False and buf.size == 3
    with pytest.raises(ValueError, match="returns were not given"):
        buf.add(frames[3:5], meas[3:5], expert[3:5], returns[3:5])
    with pytest.raises(ValueError, match="18 rows on top of 3 exceed the capacity of 20"):
        buf.add(frames[:18], meas[:18], expert[:18])
    assert buf.size == 3
    m.dev.close()


@pytest.mark.parametrize("with_returns", (True, False))
@pytest.mark.parametrize("batch_size", (4, 32))
def test_clone_is_a_host_loop_of_clone_steps(mlp_vae, tmp_path, with_returns, batch_size):
    """clone() against PpoDevice.clone_step over the same permutation on a twin policy, bitwise; at batch size 32 every epoch is one partial minibatch of 20."""
    import torch
    from ppo import ADAM_BETA1, ADAM_BETA2, _adam_alpha
    from rollout_gpu_common import flat_state, make_pair
    _, m = make_pair(tmp_path / "m", input_dim=MLP_Z + N_MEAS)
    _, twin = make_pair(tmp_path / "t", input_dim=MLP_Z + N_MEAS)
    assert bitwise(flat_state(m), flat_state(twin))
    buf, _, _, _ = filled(mlp_vae, m, with_returns)
    for kind, epochs in (("nll", 2), ("mse", 1)):
        old = m.dev.params_old.clone()
        np.random.seed(11)
        out = buf.clone(num_epochs=epochs, batch_size=batch_size, loss=kind)
        np.random.seed(11)
        want = []
        for _ in range(epochs):
            idx = np.arange(CAP)
            np.random.shuffle(idx)
            perm = torch.from_numpy(idx.astype(np.int32)).to(buf.device)
            for i in range(0, CAP, batch_size):
                mb = perm[i:i + batch_size]
                n = int(mb.numel())
                alpha = _adam_alpha(twin.current_learning_rate(), twin.beta1_power, twin.beta2_power)
                twin.dev.clone_step(None, buf.states, buf.expert_actions, buf.returns if with_returns else None, kind, mb, n, 1.0 / n, 1.0, alpha)
                twin.beta1_power, twin.beta2_power = np.float32(twin.beta1_power * np.float32(ADAM_BETA1)), np.float32(twin.beta2_power * np.float32(ADAM_BETA2))
                want.append(twin.dev.clone_losses())
        steps = epochs * -(-CAP // batch_size)
        assert out["samples"] == CAP and len(out["losses"]) == steps and out["losses"] == want
        assert set(out) == {"losses", "samples"} and set(out["losses"][0]) == {"clone_loss", "value_loss", "loss", "mean_sq_error"}
        assert bitwise(flat_state(m), flat_state(twin)) and bitwise(old, m.dev.params_old)
        assert (out["losses"][0]["value_loss"] > 0) == with_returns
    assert m.train_step_counter == (2 + 1) * -(-CAP // batch_size) and m.beta1_power == twin.beta1_power
    # with clipping on, every step's norm and factor come back as well
    m.set_max_grad_norm(0.5)
    np.random.seed(12)
    out = buf.clone(num_epochs=1, batch_size=batch_size)
    n_steps = -(-CAP // batch_size)
    assert out["grad_norms"].shape == (n_steps,) and out["clip_scales"].shape == (n_steps,) and (out["grad_norms"] > 0).all() and (out["clip_scales"] <= 1).all()
    m.dev.close()
    twin.dev.close()


def test_evaluate_against_float64_and_theta_old_is_untouched(mlp_vae, tmp_path):
    from oracle import ppo_oracle as po
    from rollout_gpu_common import flat_state, make_pair
    _, m = make_pair(tmp_path / "m", input_dim=MLP_Z + N_MEAS)
    buf, _, _, (_, _, expert, _) = filled(mlp_vae, m, False)
    m.dev.params_old.mul_(1.5)                                                       # (theta_old differs from theta: a copy would show)
    before = flat_state(m)
    ev = buf.evaluate()
    assert bitwise(before, flat_state(m))
    space = po.ActionSpace()
    th = m.dev.export_params()
    mean = bc.forward(th, buf.states.cpu().numpy(), space.low, space.high, value=False)["mean"]
    ls = th[bc.NAMES[6]].astype(np.float64)
    d = mean - expert.astype(np.float64)
    z = d / np.exp(ls)
    nll, abs_terms = (z * z / 2 + ls + bc.HALF_LOG_2PI).sum(1).mean(), (z * z / 2 + np.abs(ls) + bc.HALF_LOG_2PI).sum(1).mean()
    print("\nevaluate: nll %.9g (float64 %.9g), mean_sq_error %.9g (%.9g), max_abs_error %s (%s)" % (ev["nll"], nll, ev["mean_sq_error"], (d * d).sum(1).mean(),
                                                                                                    ev["max_abs_error"], np.abs(d).max(0)))
    assert ev["samples"] == CAP and abs(ev["nll"] - nll) <= 1e-4 * abs_terms
    assert ev["mean_sq_error"] == pytest.approx((d * d).sum(1).mean(), rel=1e-4)
    assert ev["max_abs_error"].shape == (2,) and np.allclose(ev["max_abs_error"], np.abs(d).max(0), rtol=1e-4)
    # and after training on the same rows the policy is closer to the expert
    np.random.seed(5)
    buf.clone(num_epochs=30, batch_size=20, loss="mse")
    assert buf.evaluate()["mean_sq_error"] < ev["mean_sq_error"]
    m.dev.close()


def test_frozen_observation_statistics(mlp_vae, tmp_path):
    """set_observation_normalization(state_dict): `states` within 1 fp32 ulp of normalize_observations(raw_states), raw_states bitwise what the step returned."""
    from oracle import ppo_oracle as po
    from rollout import DemonstrationBuffer, RolloutBuffer, normalize_observations
    from rollout_gpu_common import make_pair
    din = MLP_Z + N_MEAS
    _, m = make_pair(tmp_path / "m", input_dim=din)
    rng = np.random.RandomState(51)
    src = RolloutBuffer(mlp_vae, m, 2, 2, seed=3)
    src.set_observation_normalization(clip=2.5, epsilon=1e-8, frozen=True)
    sd = dict(src.observation_normalization_state(), count=100.0, mean=rng.uniform(-0.5, 0.5, din), m2=100.0 * rng.uniform(0.2, 4.0, din))
    src.load_observation_normalization_state(sd)
    sd = src.observation_normalization_state()
    buf = DemonstrationBuffer(mlp_vae, m, CAP, chunk=8, seed=3)
    buf.set_observation_normalization(sd)
    big, kept = guarded(buf), recorded(buf)
    frames, meas, expert, _ = demo_inputs(71, CAP, MLP_SRC, po.ActionSpace())
    buf.add(frames, meas, expert)
    raw, nrm = buf.raw_states.cpu().numpy(), buf.states.cpu().numpy()
    assert np.array_equal(raw, np.concatenate([k[2] for k in kept]).astype(np.float32))
    want = normalize_observations(raw, sd)
    ulp = np.spacing(np.abs(want).astype(np.float32))
    assert (np.abs(nrm.astype(np.float64) - want.astype(np.float64)) <= ulp).all() and np.abs(nrm).max() <= np.float32(2.5)
    assert not np.array_equal(raw, nrm)
    for name, b in big.items():
        assert bool((b[-8:] == SENT).all()), name
    m.dev.close()


def test_buffer_on_the_smallest_convvae(tmp_path):
    """The ConvVAE encoder at the smallest model of tests/vae_engine_cases.py (48 x 48 x 3, z = 8): 5 rows with chunk = 4."""
    import vae_engine_cases as vc
    from rollout_gpu_common import make_pair
    from vae.models import ConvVAE
    c = vc.by_id(1)
    vae = ConvVAE(np.array(vc.src_shape(c)), np.array(vc.tgt_shape(c)), z_dim=c.z, model_dir=str(tmp_path / "vae"), precision="fp32", training=False, seed=0)
    vae.set_weights(vc.params(c))
    vae.init_session(init_logging=False)
    _, m = make_pair(tmp_path / "m", input_dim=c.z + N_MEAS)
    buf, big, kept, (_, meas, expert, returns) = filled(vae, m, True, src=vc.src_shape(c), seed=72, chunk=4, capacity=5, parts=(5,))
    assert [len(k[1]) for k in kept] == [4, 1]
    s = np.concatenate([k[2] for k in kept])
    assert np.array_equal(buf.states.cpu().numpy(), s.astype(np.float32)) and np.array_equal(s[:, c.z:], meas)
    assert np.array_equal(buf.expert_actions.cpu().numpy(), expert) and np.array_equal(buf.returns.cpu().numpy(), returns)
    for name, b in big.items():
        assert bool((b[-8:] == SENT).all()), name
    np.random.seed(3)
    out = buf.clone(num_epochs=2, batch_size=4)
    assert len(out["losses"]) == 4 and all(np.isfinite(list(rec.values())).all() for rec in out["losses"])
    assert np.isfinite(buf.evaluate()["nll"])
    m.dev.close()
    vae.dev.close()
