"""Global-norm gradient clipping on the GPU (mi_ppo_grad_norm, the clipped mi_ppo_apply_adam / mi_ppo_train_step[_idx|_dp], PPO.set_max_grad_norm and the rollout
buffer's grad_norms).  Engine as test_c_c3_ppo_gpu.make_pair builds it (input 67, 2 actions, hidden 500 / 300), theta perturbed by 0.02 so that ratios differ from 1;
minibatches of M = 5 (one partial loss block), 32, 256 and 257 (two row chunks, the slab-sum route).

The reference is always existing code, never the new kernels: the gradient buffer as the existing route leaves it, numpy float64 over export_grads() for the norm, a
torch multiply of the buffer by the fp32 factor, the existing apply_adam with clipping off.  The gradient comes from forward_backward for the forms whose step runs
the same kernels on the same operands (train_step, train_step_idx without a log pi_old cache).  A step with the CACHED log pi_old is not bitwise forward_backward's:
the cache (mi_ppo_logp_old) and the in-step old-policy forward differ in the last bits (tests/test_m_rollout_buffer_gpu.py measured 5.2e-7 on the parameters), so for
those forms the gradient is taken from the existing one-call step itself: with alpha = 0, beta1 = 0 and zero Adam slots, m <- m + (g - m) * 1 leaves adam_m = g
exactly and the parameters where they were, at every M, through the in-tile Adam as through the flat one.

1. grad_norm alone: against float32(norm_ref) within 2 fp32 ulps (2.4e-7 relative: the double sums differ from numpy's by summation order only, ~1e-16, so the fp32
   values can differ only across a rounding boundary), the factor, bitwise repeat, nothing else written, alignment gaps do not count, the all-zero gradient.
2. the clipped step is the reference route, bit for bit: each M, both precisions, the three forms, c = 0.5 / 2 x the norm and inf; c = inf against the in-tile Adam.
3. off is off.   4. routes: the per-layer path, ensure_batch, the data-parallel call on a recording communicator.   5. a RolloutBuffer update end to end."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import ppo_oracle as po  # noqa: E402
from rollout_gpu_common import bitwise, inputs, make_pair, make_world, rel_err  # noqa: E402

MS = (5, 32, 256, 257)
ULP2 = 2.4e-7                                            # 2 fp32 ulps, relative
ALPHA = 1e-4
SENTINEL = -777.0


def perturbed(tmp, precision=None, input_dim=67):
    """make_pair with theta != theta_old: theta perturbed by 0.02 (theta_old stays the initial copy), as test_c_c3_ppo_gpu's fused-step case."""
    o, m = make_pair(tmp, input_dim=input_dim, precision=precision)
    rng = np.random.RandomState(5)
    for k in o.params:
        o.params[k] = o.params[k] + (0.02 * rng.standard_normal(o.params[k].shape)).astype(np.float32)
    m.dev.load_params(o.params)
    return m


def batch(m, M, input_dim=67, seed=None):
    rng = np.random.RandomState(5 + M if seed is None else seed)
    s = (0.5 * rng.standard_normal((M, input_dim))).astype(np.float32)
    a = np.stack([rng.uniform(-1, 1, M), rng.uniform(0, 1, M)], axis=1).astype(np.float32)
    R, A = rng.randn(M).astype(np.float32), rng.randn(M).astype(np.float32)
    return s, a, R, A


def to_dev(m, host):
    s, a, R, A = host
    M = len(s)
    return m._to_dev(s, s.shape), m._to_dev(a, a.shape), m._to_dev(R, (M,)), m._to_dev(A, (M,))


class State:
    """params / adam_m / adam_v of an engine, to start several routes from the same point."""

    def __init__(self, d):
        self.saved = [x.clone() for x in (d.params, d.adam_m, d.adam_v)]

    def restore(self, d):
        for x, y in zip((d.params, d.adam_m, d.adam_v), self.saved):
            x.copy_(y)
        d.grads.zero_()


def result(d):
    return [x.clone() for x in (d.params, d.adam_m, d.adam_v)]


def gap_mask(d):
    import torch
    used = torch.zeros(d.n_flat, dtype=torch.bool, device=d.device)
    for _, (o, s) in d.layout.items():
        used[o:o + s] = True
    return ~used


def norm_ref_of(d):
    """numpy float64 over the 13 variables of the gradient buffer (export_grads: no alignment gaps, no padded rows)."""
    g = d.export_grads()
    return float(np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in g.values())))


class Engine:
    def __init__(self, tmp, precision):
        self.m = perturbed(tmp, precision)
        self.d = self.m.dev
        self.d.ensure_batch(257)                         # the engine is recreated once, before any state is snapshotted
        self.state0 = State(self.d)
        self.gaps = gap_mask(self.d)
        self.data = {M: to_dev(self.m, batch(self.m, M)) for M in MS}
        self._ref = {}

    def gradient(self, M, form):
        """The gradient buffer the EXISTING code forms for this step form from state0 (clipping off) -> (flat buffer with 4.25 in the gaps, norm_ref).  Computed once."""
        import torch
        key = (M, form)
        if key not in self._ref:
            d = self.d
            s, a, R, A = self.data[M]
            self.state0.restore(d)
            d.set_max_grad_norm(None)
            if form in ("plain", "idx"):                 # the same kernels on the same operands as forward_backward (idx: the shuffled rows of a table, gathered here)
                d.grads.fill_(4.25)
                d.forward_backward(s, a, R, A, M, 1.0 / M, 1.0)
            else:                                        # cached log pi_old: adam_m of the existing one-call step with alpha = 0, beta1 = 0 from zero slots IS the gradient
                d.adam_m.zero_(); d.adam_v.zero_()
                before = d.params.clone()
                lp, tab = self.cache(M)
                if form == "cached":
                    d.train_step(s, a, R, A, M, 1.0 / M, 1.0, 0.0, beta1=0.0, logp_old=lp)
                else:
                    ts, ta, tR, tA, tlp, rows = tab
                    d.train_step_idx(ts, ta, tR, tA, tlp, rows, M, 1.0 / M, 1.0, 0.0, beta1=0.0)
                assert torch.equal(d.params.view(torch.int32)[~self.gaps], before.view(torch.int32)[~self.gaps])
                d.grads.copy_(d.adam_m)
                if M <= 256:                             # the in-tile Adam leaves the alignment gaps alone, and so does the gradient chain: they hold what clipped() puts
                    d.grads[self.gaps] = 4.25            # there.  Above 256 rows the slab sum writes the gaps too, and the flat Adam left that in adam_m as well
            g = d.grads.clone()
            self._ref[key] = (g, norm_ref_of(d))
            self.state0.restore(d)
        return self._ref[key]

    def cache(self, M):
        """log pi_old of the minibatch's samples, and the minibatch as shuffled rows of a table of max(64, M) rows (the other rows hold other samples)."""
        import torch
        key = ("cache", M)
        if key not in self._ref:
            d = self.d
            s, a, R, A = self.data[M]
            lp = torch.empty(M, device=d.device)
            d.logp_old(s, a, M, lp)
            n = max(64, M)
            rows = np.random.RandomState(M).permutation(n)[:M].astype(np.int32)
            fill = to_dev(self.m, batch(self.m, n, seed=1000 + M))
            tab = [x.clone() for x in fill] + [torch.zeros(n, device=d.device)]
            rd = torch.from_numpy(rows).to(d.device)
            for t, x in zip(tab, (s, a, R, A, lp)):
                t[rd.long()] = x
            self._ref[key] = (lp, tab + [rd])
        return self._ref[key]

    def clipped(self, M, form, c):
        """The clipped step of this form from state0 -> (params / m / v, buffer 2, gradient buffer afterwards)."""
        d = self.d
        s, a, R, A = self.data[M]
        self.state0.restore(d)
        d.grads.fill_(4.25)
        d.set_max_grad_norm(c)
        lp, tab = self.cache(M)
        ts, ta, tR, tA, tlp, rows = tab
        if form == "plain":
            d.train_step(s, a, R, A, M, 1.0 / M, 1.0, ALPHA)
        elif form == "cached":
            d.train_step(s, a, R, A, M, 1.0 / M, 1.0, ALPHA, logp_old=lp)
        elif form == "idx":
            d.train_step_idx(ts, ta, tR, tA, None, rows, M, 1.0 / M, 1.0, ALPHA)
        else:
            d.train_step_idx(ts, ta, tR, tA, tlp, rows, M, 1.0 / M, 1.0, ALPHA)
        out = result(d), d.grad_clip.clone(), d.grads.clone()
        d.set_max_grad_norm(None)
        return out

    def reference(self, grad, scale):
        """state0, the gradient buffer multiplied by the fp32 factor with torch (scale None: no multiply at all), the existing apply_adam."""
        d = self.d
        self.state0.restore(d)
        d.set_max_grad_norm(None)
        d.grads.copy_(grad)
        if scale is not None:
            d.grads.mul_(scale)                          # a 0-dim fp32 device tensor: one fp32 multiply per element
        d.apply_adam(ALPHA)
        return result(d), d.grads.clone()


@pytest.fixture(scope="module")
def engines(tmp_path_factory):
    made = {}

    def get(precision):
        if precision not in made:
            made[precision] = Engine(tmp_path_factory.mktemp("clip_" + precision), precision)
        return made[precision]
    return get


def check_record(rec, norm_ref, c, tag):
    """buffer 2 {norm, scale, c, 0} against the float64 reference -> (norm, scale) as float32."""
    rec = rec.cpu().numpy()
    norm, scale = rec[0], rec[1]
    print("%s: norm %.9g (float64 reference %.17g, relative distance %.2e), scale %.9g" % (tag, norm, norm_ref, abs(float(norm) - norm_ref) / norm_ref, scale))
    assert abs(float(norm) - float(np.float32(norm_ref))) <= ULP2 * norm_ref, (tag, norm, norm_ref)
    assert rec[2] == np.float32(c) and rec[3] == 0.0, (tag, rec)
    if norm_ref > c:
        want = float(np.float32(c / norm_ref))
        assert abs(float(scale) - want) <= ULP2 * want and scale < 1.0, (tag, scale, want)
    else:
        assert scale == np.float32(1.0), (tag, scale)
    return norm, scale


@pytest.mark.parametrize("M", MS)
def test_grad_norm_alone(engines, M):
    import torch
    e = engines("fp32")
    d = e.d
    grad, norm_ref = e.gradient(M, "plain")
    assert norm_ref > 1e-3
    d.grads.copy_(grad)
    d.grads[e.gaps] = 0.0
    d.grad_clip.fill_(SENTINEL)
    before = [x.clone() for x in (d.params, d.params_old, d.adam_m, d.adam_v, d.grads, d.losses, d.action_mean)]
    recs = {}
    for name, c in (("clips", 0.5 * norm_ref), ("above", 2 * norm_ref), ("inf", float("inf"))):
        d.grad_norm(c)
        recs[name] = d.grad_clip.clone()
        check_record(recs[name], norm_ref, c, "M = %d, %s" % (M, name))
        d.grad_norm(c)
        assert torch.equal(d.grad_clip.view(torch.int32), recs[name].view(torch.int32)), name          # two calls: bitwise equal
    assert bitwise([x for x in (d.params, d.params_old, d.adam_m, d.adam_v, d.grads, d.losses, d.action_mean)], before)
    assert d.engine_max_grad_norm() == 0.0                                                              # the engine's setting is not touched either
    # the alignment gaps do not count
    assert int(e.gaps.sum()) >= 6 + 6 + 7                                            # at least those behind the action bias, action_logstd and the value bias
    d.grads[e.gaps] = 1e6
    d.grad_norm(0.5 * norm_ref)
    assert torch.equal(d.grad_clip.view(torch.int32), recs["clips"].view(torch.int32))
    if M == 5:
        # an all-zero gradient: norm 0, scale 1, no NaN
        d.grads.zero_()
        for c in (0.5, float("inf")):
            d.grad_norm(c)
            assert d.grad_clip.cpu().numpy().tolist() == [0.0, 1.0, c, 0.0]
        # a non-finite norm is reported as it is and leaves the gradient alone
        d.grads[3] = float("inf")
        d.grad_norm(0.5)
        rec = d.grad_clip.cpu().numpy()
        assert np.isinf(rec[0]) and rec[1] == 1.0
        d.grads[3] = float("nan")
        d.grad_norm(0.5)
        rec = d.grad_clip.cpu().numpy()
        assert np.isnan(rec[0]) and rec[1] == 1.0
    e.state0.restore(d)


@pytest.mark.parametrize("form", ["plain", "cached", "idx", "idx_cached"])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("M", MS)
def test_clipped_step_is_the_reference_route_bit_for_bit(engines, M, precision, form):
    import torch
    e = engines(precision)
    d = e.d
    assert d.precision == precision
    grad, norm_ref = e.gradient(M, form)
    tag = "M = %d, %s, %s" % (M, precision, form)
    # c = 0.5 x the norm: clipped
    c = 0.5 * norm_ref
    got, rec, after = e.clipped(M, form, c)
    norm, scale = check_record(rec, norm_ref, c, tag)
    assert scale < 1.0
    want, after_ref = e.reference(grad, rec[1])
    assert bitwise(got, want), tag
    assert not bool(after.any()) and not bool(after_ref.any())                       # the gradient buffer is all zeros afterwards, gaps included
    again, rec2, _ = e.clipped(M, form, c)
    assert bitwise(again, got) and torch.equal(rec2.view(torch.int32), rec.view(torch.int32)), tag      # two runs from the same state
    # c = 2 x the norm and c = inf: the factor is exactly 1 and the result is the unscaled gradient through apply_adam, without any multiply
    plain_adam, _ = e.reference(grad, None)
    assert not bitwise(plain_adam, got)
    for c in (2 * norm_ref, float("inf")):
        got1, rec1, after1 = e.clipped(M, form, c)
        check_record(rec1, norm_ref, c, tag)
        assert rec1[1].item() == 1.0 and bitwise(got1, plain_adam) and not bool(after1.any()), (tag, c)
    # c = inf against the unclipped one-call step (the in-tile Adam at M <= 256) on the same inputs: test_c_c3_ppo_gpu's tolerance between its two forms
    e.state0.restore(d)
    s, a, R, A = e.data[M]
    lp, (ts, ta, tR, tA, tlp, rows) = e.cache(M)
    if form == "plain":
        d.train_step(s, a, R, A, M, 1.0 / M, 1.0, ALPHA)
    elif form == "cached":
        d.train_step(s, a, R, A, M, 1.0 / M, 1.0, ALPHA, logp_old=lp)
    else:
        d.train_step_idx(ts, ta, tR, tA, None if form == "idx" else tlp, rows, M, 1.0 / M, 1.0, ALPHA)
    one_call = result(d)
    used = ~e.gaps
    print("%s: c = inf against the unclipped one-call step: bitwise %s, max |diff| of the parameters %.3e" %
          (tag, bitwise([x[used] for x in got1], [x[used] for x in one_call]), float((got1[0][used] - one_call[0][used]).abs().max())))
    assert np.allclose(got1[0][used].cpu().numpy(), one_call[0][used].cpu().numpy(), rtol=0, atol=1e-7), tag
    e.state0.restore(d)


def test_off_is_off(tmp_path):
    import torch
    m_a, m_b = perturbed(tmp_path / "a"), perturbed(tmp_path / "b")
    host = batch(m_a, 32)
    outs = []
    for m, touch in ((m_a, True), (m_b, False)):
        d = m.dev
        if touch:
            m.set_max_grad_norm(0.5)
            assert d.engine_max_grad_norm() == 0.5
            m.set_max_grad_norm(None)
        assert d.engine_max_grad_norm() == 0.0
        d.grad_clip.fill_(SENTINEL)
        s, a, R, A = to_dev(m, host)
        d.train_step(s, a, R, A, 32, 1.0 / 32, 1.0, ALPHA)
        d.forward_backward(s, a, R, A, 32, 1.0 / 32, 1.0)
        d.apply_adam(ALPHA)
        assert bool((d.grad_clip == SENTINEL).all())                                 # buffer 2 is not written
        outs.append(result(d))
    assert bitwise(outs[0], outs[1])


def test_per_layer_path(tmp_path):
    """input_dim 100: the padded width 104 is above the fused range, so forward_backward and the step run per layer, and the clipping arrives through apply_adam."""
    m = perturbed(tmp_path, input_dim=100)
    d = m.dev
    assert not d.fused_ok()
    M = 5
    host = batch(m, M, input_dim=100)
    s, a, R, A = to_dev(m, host)
    state0 = State(d)
    d.forward_backward(s, a, R, A, M, 1.0 / M, 1.0)
    grad, norm_ref = d.grads.clone(), norm_ref_of(d)
    c = 0.5 * norm_ref
    state0.restore(d)
    m.set_max_grad_norm(c)
    m.train_step(*host)                                                              # PPO.train_step: numpy in, one clipped SGD step
    got, rec = result(d), d.grad_clip.clone()
    norm, scale = check_record(rec, norm_ref, c, "per-layer path")
    assert m.last_grad_norm() == {"grad_norm": float(norm), "clip_scale": float(scale)}
    assert not bool(d.grads.any())
    state0.restore(d)
    m.set_max_grad_norm(None)
    d.grads.copy_(grad)
    d.grads.mul_(rec[1])
    from ppo import _adam_alpha
    d.apply_adam(_adam_alpha(1e-4, 0.9, 0.999))                                      # PPO.train's step size: make_pair's learning rate, the first Adam step
    assert bitwise(result(d), got)


def test_setting_survives_ensure_batch(tmp_path):
    m = perturbed(tmp_path)
    d = m.dev
    assert d.max_batch == 256
    M = 257
    s, a, R, A = to_dev(m, batch(m, M))
    state0 = State(d)
    m.set_max_grad_norm(1e-3)                                                        # far below any norm of this case
    handle = d.handle
    d.train_step(s, a, R, A, M, 1.0 / M, 1.0, ALPHA)                                 # ensure_batch recreates the engine for the larger batch
    assert d.handle != handle and d.max_batch >= M and d.engine_max_grad_norm() == float(np.float32(1e-3))
    got, rec = result(d), d.grad_clip.clone()
    assert rec[2].item() == float(np.float32(1e-3)) and 0 < rec[1].item() < 1.0
    state0.restore(d)
    m.set_max_grad_norm(None)
    d.forward_backward(s, a, R, A, M, 1.0 / M, 1.0)
    check_record(rec, norm_ref_of(d), 1e-3, "after ensure_batch")
    d.grads.mul_(rec[1])
    d.apply_adam(ALPHA)
    assert bitwise(result(d), got)


def test_data_parallel_call_on_a_recording_communicator(tmp_path):
    """mi_ppo_train_step_dp at world size 1 with a communicator that records instead of communicating (as bench.py's data_parallel_form_at_one_rank builds it):
    the norm is taken behind the all-reduce, the clipped call is the reference route bit for bit."""
    m = perturbed(tmp_path)
    d = m.dev
    M = 32
    s, a, R, A = to_dev(m, batch(m, M))
    hcomm, log = ctypes.c_void_p(), np.zeros((64, 4), np.int64)
    d.L.mi_comm_init_recording(ctypes.addressof(hcomm), 0, 1, log.ctypes.data, 64)
    try:
        state0 = State(d)
        d.forward_backward(s, a, R, A, M, 1.0 / M, 1.0)
        grad, norm_ref = d.grads.clone(), norm_ref_of(d)
        c = 0.5 * norm_ref
        state0.restore(d)
        m.set_max_grad_norm(c)
        d.train_step_dp(hcomm, s, a, R, A, None, None, M, 1.0 / M, 1.0, ALPHA)
        got, rec = result(d), d.grad_clip.clone()
        check_record(rec, norm_ref, c, "train_step_dp")
        assert int(d.L.mi_comm_recorded(hcomm)) == 1 and not bool(d.grads.any())
        state0.restore(d)
        m.set_max_grad_norm(None)
        d.grads.copy_(grad)
        d.grads.mul_(rec[1])
        d.apply_adam(ALPHA)
        assert bitwise(result(d), got)
    finally:
        d.L.mi_comm_destroy(hcomm)


# ---- end to end: a RolloutBuffer of 4 environments x 8 steps, scripted frames ----
E, T, BATCH, EPOCHS, SEED = 4, 8, 8, 2, 3
# Parameters after the update, the buffer (cached log pi_old, gather inside the kernels) against a loop of PPO.train_step calls on the same minibatches (in-step
# old-policy forward): tests/test_m_rollout_buffer_gpu.py's bound for that comparison, 4 x its measured 5.223e-07 of each tensor's max
PARAM_REL = 4 * 5.223e-07


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return make_world(tmp_path_factory, "grad_clip", policy=False)


def collect(world, tmp, source):
    """A policy and a full E x T collection through the buffer's own step; the device tables are those of the first collection (the recording step's split-K layers
    end in fp32 atomics, so two collections of the same frames can differ in the last bit)."""
    from rollout import RolloutBuffer
    _, m = make_pair(tmp)
    buf = RolloutBuffer(world["vae"], m, E, T)
    rng = np.random.RandomState(571)
    buf.reset()
    for _ in range(T):
        f, ms, nz = inputs(rng, E)
        buf.step(f, ms, noise=nz)
        buf.outcome(rng.uniform(0, 1, E), np.zeros(E, bool))
    f, ms, _ = inputs(rng, E)
    buf.bootstrap(f, ms)
    mine = [buf.states, buf.actions, buf.values]
    if not source:
        source.extend(x.clone() for x in mine)
    for x, y in zip(mine, source):
        x.copy_(y)
    np.random.seed(SEED)
    return m, buf


def test_rollout_buffer_update_end_to_end(world, tmp_path):
    source = []
    n_steps = EPOCHS * (E * T // BATCH)
    clip_keys = {"grad_norms", "clip_scales"}
    # the unclipped twin: inf measures every step's norm and never clips
    m0, b0 = collect(world, tmp_path / "w0", source)
    m0.set_max_grad_norm(float("inf"))
    out0 = b0.update(num_epochs=EPOCHS, batch_size=BATCH)
    assert out0["grad_norms"].shape == (n_steps,) and out0["grad_norms"].dtype == np.float32 and np.all(out0["clip_scales"] == 1.0)
    assert np.all(np.isfinite(out0["grad_norms"])) and np.all(out0["grad_norms"] > 0)
    c = 0.5 * float(out0["grad_norms"][0])
    # clipped
    m1, b1 = collect(world, tmp_path / "w1", source)
    m1.set_max_grad_norm(c)
    out1 = b1.update(num_epochs=EPOCHS, batch_size=BATCH)
    assert set(out1) - clip_keys == set(out0) - clip_keys
    for k in ("grad_norms", "clip_scales"):
        assert out1[k].shape == (n_steps,) and out1[k].dtype == np.float32, k
    assert out1["grad_norms"][0] == out0["grad_norms"][0] and out1["clip_scales"][0] < 1.0       # the first step starts from the same parameters
    assert out1["clip_scales"][0] == pytest.approx(0.5, rel=1e-6)
    assert m1.last_grad_norm() == {"grad_norm": float(out1["grad_norms"][-1]), "clip_scale": float(out1["clip_scales"][-1])}
    p0, p1 = m0.dev.export_params(), m1.dev.export_params()
    assert max(rel_err(p1[k], p0[k]) for k in p0) > 1e-6                             # the parameters differ from the unclipped twin's
    # a loop of clipped PPO.train_step calls on the same minibatches
    _, m2 = make_pair(tmp_path / "w2")
    m2.set_max_grad_norm(c)
    valid = b1.rows.valid_rows()
    s, a = b1.states.cpu().numpy()[valid], b1.actions.cpu().numpy()[valid]
    ret, adv = b1.returns.cpu().numpy()[valid], b1.advantages.cpu().numpy()[valid]
    m2.update_old_policy()
    np.random.seed(SEED)
    norms2 = []
    for mb in po.minibatch_schedule(len(valid), BATCH, EPOCHS):
        m2.train_step(s[mb], a[mb], ret[mb], adv[mb])
        norms2.append(m2.last_grad_norm())
    p2 = m2.dev.export_params()
    worst = max(rel_err(p1[k], p2[k]) for k in p1)
    print("\nclipped update, buffer against a loop of clipped PPO.train_step calls: max |diff| / tensor max = %.3e; norms %s, factors %s" %
          (worst, out1["grad_norms"], out1["clip_scales"]))
    assert worst <= PARAM_REL, worst
    # (the norm is a smooth function of parameters that agree to 2e-6 of each tensor's max and of a log pi_old that agrees to fp32 rounding: 1e-3 is far outside that)
    assert np.allclose([n["grad_norm"] for n in norms2], out1["grad_norms"], rtol=1e-3) and np.allclose([n["clip_scale"] for n in norms2], out1["clip_scales"], rtol=1e-3)
    # update_with_diagnostics: per-epoch records consistent with the arrays
    m3, b3 = collect(world, tmp_path / "w3", source)
    m3.set_max_grad_norm(c)
    out3 = b3.update_with_diagnostics(num_epochs=EPOCHS, batch_size=BATCH)
    assert np.array_equal(out3["grad_norms"], out1["grad_norms"]) and np.array_equal(out3["clip_scales"], out1["clip_scales"])
    per = n_steps // EPOCHS
    for i, rec in enumerate(out3["epochs"]):
        assert rec["grad_norm_max"] == float(out3["grad_norms"][i * per:(i + 1) * per].max())
        assert rec["clipped_steps"] == int((out3["clip_scales"][i * per:(i + 1) * per] < 1.0).sum())
    assert out3["epochs"][0]["clipped_steps"] >= 1 and len(out3["epochs"]) == EPOCHS
    # with the setting off none of the keys appears
    m4, b4 = collect(world, tmp_path / "w4", source)
    assert m4.max_grad_norm is None
    out4 = b4.update_with_diagnostics(num_epochs=EPOCHS, batch_size=BATCH)
    assert not clip_keys & set(out4) and all("grad_norm_max" not in rec and "clipped_steps" not in rec for rec in out4["epochs"])
    assert set(out4) == set(out3) - clip_keys
