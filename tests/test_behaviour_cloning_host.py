"""Host side of behaviour cloning (no GPU): the numpy reference of behaviour_cloning_cases.py against central differences and on a teacher-labelled set, the C ABI's
new entry, and the refusals of PPO.clone_step and DemonstrationBuffer.add, which raise before a device is touched."""
import ctypes
import types

import numpy as np
import pytest

import behaviour_cloning_cases as bc
from oracle import ppo_oracle as po

FD_REL = 1e-6


def small_problem(seed=4, M=7, din=5, A=3, hidden=(12, 8)):
    rng = np.random.RandomState(seed)
    low, high = bc.bounds(A)
    th = bc.init_theta(rng, din, A, hidden)
    cand = (0.5 * rng.standard_normal((8 * M, din))).astype(np.float32)
    s = cand[~bc.near_relu_kink(th, cand, low, high, tau=1e-2)][:M]                  # (far from every kink: a central difference must not step across one)
    assert len(s) == M
    a = rng.uniform(low, high, (M, A)).astype(np.float32)
    R = rng.standard_normal(M).astype(np.float32)
    return th, s, a, R, low, high


@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("with_returns", (True, False))
def test_analytic_gradients_against_central_differences(kind, with_returns):
    """Every entry of all 13 tensors: |analytic - (L(x + h) - L(x - h)) / 2 h| <= 1e-6 of the tensor's largest gradient (float64, h = 1e-6 max(1, |x|))."""
    th, s, a, R, low, high = small_problem()
    R = R if with_returns else None
    th = {k: v.astype(np.float64) for k, v in th.items()}
    _, g, _, _ = bc.loss_and_grads(th, s, a, R, kind, low, high)
    for name in bc.NAMES:
        num = np.zeros_like(th[name])
        it = np.nditer(th[name], flags=["multi_index"])
        for x in it:
            i = it.multi_index
            h = 1e-6 * max(1.0, abs(float(x)))
            up, dn = dict(th), dict(th)
            up[name], dn[name] = th[name].copy(), th[name].copy()
            up[name][i] += h
            dn[name][i] -= h
            num[i] = (bc.loss_and_grads(up, s, a, R, kind, low, high)[0]["loss"] - bc.loss_and_grads(dn, s, a, R, kind, low, high)[0]["loss"]) / (2 * h)
        scale = max(np.abs(num).max(), np.abs(g[name]).max())
        if scale == 0.0:                                                             # the value net without returns, logstd under "mse": both are exactly zero
            assert not g[name].any() and not num.any(), name
            assert name in bc.VALUE_NET or name == bc.NAMES[6], name
            continue
        assert np.abs(g[name] - num).max() <= FD_REL * scale, (name, float(np.abs(g[name] - num).max() / scale))


def test_mse_gives_a_logstd_gradient_of_exactly_zero():
    for shape in ("A2", "A3"):
        for wr in (True, False):
            _, g, _, _ = bc.reference(shape, 33, "mse", wr)
            assert g[bc.NAMES[6]].shape == (bc.SHAPES[shape][1],) and not g[bc.NAMES[6]].any()
            _, g32, _, _ = bc.reference(shape, 33, "mse", wr, dtype=np.float32)
            assert not g32[bc.NAMES[6]].any()
    _, g, _, _ = bc.reference("A2", 33, "nll", False)
    assert g[bc.NAMES[6]].all() and not any(g[k].any() for k in bc.VALUE_NET)        # "nll" does move logstd; policy only leaves the value net's gradients at zero


@pytest.mark.parametrize("kind", bc.KINDS)
def test_200_reference_steps_lower_the_mean_squared_error(kind):
    """A teacher-labelled set (the expert IS a policy of the same family, no noise): 200 reference steps with TF-Adam lower mean_sq_error."""
    rng = np.random.RandomState(12)
    din, A, hidden, M = 5, 3, (36, 20), 64
    low, high = bc.bounds(A)
    c = bc.Case()
    c.theta, teacher = bc.init_theta(rng, din, A, hidden), bc.init_theta(rng, din, A, hidden)
    c.s = (0.5 * rng.standard_normal((M, din))).astype(np.float32)
    c.a = bc.forward(teacher, c.s, low, high, value=False)["mean"].astype(np.float32)
    c.R, c.low, c.high = np.zeros(M, np.float32), low, high
    before = bc.loss_and_grads(c.theta, c.s, c.a, None, kind, low, high)[0]
    after = bc.loss_and_grads(bc.trajectory(c, kind, False, 200), c.s, c.a, None, kind, low, high)[0]
    assert after["mean_sq_error"] < 0.5 * before["mean_sq_error"], (before, after)
    assert after["clone_loss"] < before["clone_loss"]


def test_the_library_exports_the_entry_with_the_headers_prototype():
    from mi355 import lib as milib
    protos = milib.parse_header()
    cdll = ctypes.CDLL(milib.LIB_PATH)
    assert "mi_ppo_clone_step" in protos and cdll.mi_ppo_clone_step is not None
    ret, args = protos["mi_ppo_clone_step"]
    assert ret == "int"
    assert [n for _, n in args] == ["h", "comm", "stream", "states", "expert_actions", "returns", "kind", "row_idx", "n_rows", "M", "inv_m", "grad_scale", "adam",
                                    "alpha", "beta1", "beta2", "epsilon"]
    assert [t for t, _ in args] == ["void*", "void*", "void*", "const float*", "const float*", "const float*", "int", "const int*", "int", "int", "float", "float",
                                    "int", "float", "float", "float", "float"]
    text = open(milib.HEADER).read()
    assert "[0] clone_loss   [1] value_loss" in text and "[4] mean_sq_error" in text      # the header states where the losses sit
    cdll.mi_last_error.restype = ctypes.c_char_p
    fn = cdll.mi_ppo_clone_step
    fn.restype = ctypes.c_int
    fn.argtypes = [milib._CTYPES[t] for t, _ in args]
    assert fn(*[None if t is ctypes.c_void_p else 1 for t in fn.argtypes]) == -4 and b"mi_ppo_clone_step: null handle" in cdll.mi_last_error()      # MI_ERR_STATE


def test_loss_names():
    from mi355.lib import clone_kind
    assert clone_kind("nll") == 0 and clone_kind("mse") == 1 and clone_kind(0) == 0 and clone_kind(np.int32(1)) == 1
    for bad in ("NLL", "l2", None, 2, -1, True, 0.0, ["nll"]):
        with pytest.raises(ValueError, match='who: the loss is "nll"'):
            clone_kind(bad, "who")


def make(tmp_path, din=67, **kw):
    from ppo import PPO
    return PPO(np.array([din]), po.ActionSpace(), model_dir=str(tmp_path), seed=1, **kw)


def test_clone_step_refuses_before_a_device_is_touched(tmp_path, monkeypatch):
    monkeypatch.delenv("MI355_PPO_FUSED", raising=False)
    monkeypatch.delenv("MI355_PPO_WIDE_INPUTS", raising=False)
    m = make(tmp_path)
    A = m.num_actions
    s, a = np.zeros((4, 67), np.float32), np.zeros((4, A), np.float32)
    bad_a = a.copy()
    bad_a[2, 0] = np.nan
    inf_a = a.copy()
    inf_a[0, A - 1] = np.inf
    for args, kw, text in (((s, a), dict(loss="huber"), 'PPO.clone_step: the loss is "nll"'),
                           ((s, a), dict(loss=None), 'PPO.clone_step: the loss is "nll"'),
                           ((s[:, :66], a), {}, "input_states has shape"),
                           ((s[0], a), {}, "input_states has shape"),
                           ((s[:0], a[:0]), {}, "input_states has shape"),
                           ((s, a[:3]), {}, "expert_actions has shape"),
                           ((s, a[:, :1]), {}, "expert_actions has shape"),
                           ((s, bad_a), {}, "not finite"),
                           ((s, inf_a), {}, "not finite"),
                           ((s, a), dict(returns=np.zeros(3)), "returns has shape"),
                           ((s, a), dict(learning_rate=0.0), "learning_rate"),
                           ((s, a), dict(learning_rate=float("nan")), "learning_rate")):
        with pytest.raises(ValueError, match=text):
            m.clone_step(*args, **kw)
    # the first thing a well-formed call needs is the device
    with pytest.raises(RuntimeError, match="init_session"):
        m.clone_step(s, a)
    assert m.dev is None and m.train_step_counter == 0 and m.beta1_power == np.float32(0.9)
    # a policy outside the fused range: the message points to set_wide_inputs(); with it on, the same call gets as far as the missing device
    w = make(tmp_path, din=131)
    sw = np.zeros((4, 131), np.float32)
    with pytest.raises(ValueError, match=r"PPO.clone_step: behaviour cloning exists only in the fused kernels .*PPO.set_wide_inputs\(\)"):
        w.clone_step(sw, a)
    with pytest.raises(ValueError, match=r"PPO._clone_rows: behaviour cloning exists only in the fused kernels"):
        w._clone_rows(None, None, None, None, 4, 4)
    w.set_wide_inputs()
    with pytest.raises(RuntimeError, match="init_session"):
        w.clone_step(sw, a)
    monkeypatch.setenv("MI355_PPO_FUSED", "0")
    with pytest.raises(ValueError, match="MI355_PPO_FUSED=0"):
        m.clone_step(s, a)
    assert w.dev is None


class _NoDevice:
    """Stands where a step class or a device table would: any use of it is a launch."""

    def __getattr__(self, name):
        raise AssertionError("a refused add() reached the device: " + name)


def host_buffer(capacity=20, size=0, has_returns=None, A=2, n_meas=3, frame_bytes=72):
    """A DemonstrationBuffer as check_add() sees it, built without a device."""
    from rollout import DemonstrationBuffer
    b = DemonstrationBuffer.__new__(DemonstrationBuffer)
    b.capacity, b.size, b.has_returns, b.A = capacity, size, has_returns, A
    step = types.SimpleNamespace(frame_bytes=frame_bytes, n_meas=n_meas, record=_NoDevice())
    b._step = step
    space = po.ActionSpace()
    b.ppo = types.SimpleNamespace(action_low=np.asarray(space.low, np.float32), action_high=np.asarray(space.high, np.float32), num_actions=A)
    b.states = b.policy_actions = b.policy_values = b.expert_actions = b.returns = _NoDevice()
    b.raw_states = None
    return b


def test_add_refuses_by_name_before_any_launch():
    b = host_buffer()
    lo, hi = b.ppo.action_low, b.ppo.action_high
    n = 7
    f = np.zeros((n, 72), np.uint8)
    meas = np.zeros((n, 3))
    a = np.tile((0.5 * (lo + hi))[None, :], (n, 1)).astype(np.float32)
    f2, n2, meas2, a2, r2 = b.check_add(f, meas, a, None)                            # a well-formed call passes the checks
    assert n2 == n and a2.dtype == np.float32 and r2 is None and np.array_equal(a2, a)
    over, nan_a, under = a.copy(), a.copy(), a.copy()
    over[3, 0] = hi[0] + 1e-3
    under[6, 1] = lo[1] - 1e-3
    nan_a[0, 1] = np.nan
    for args, text in (((np.zeros((21, 72), np.uint8), np.zeros((21, 3)), np.tile(a[:1], (21, 1)), None), "21 rows on top of 0 exceed the capacity of 20"),
                       ((f.astype(np.float32), meas, a, None), "expected uint8 frames"),
                       ((f[:, :71], meas, a, None), "expected uint8 frames"),
                       ((f, meas[:, :2], a, None), "expected measurements"),
                       ((f, meas, a[:, :1], None), "expected expert_actions"),
                       ((f, meas, nan_a, None), "expert_actions holds values that are not finite"),
                       ((f, meas, over, None), r"expert_actions outside \[action_low, action_high\]"),
                       ((f, meas, under, None), r"expert_actions outside \[action_low, action_high\]"),
                       ((f, meas, a, np.zeros(6)), "expected returns"),
                       ((f, meas, a, np.full(n, np.inf)), "returns holds values that are not finite")):
        with pytest.raises(ValueError, match="DemonstrationBuffer.add: " + text):
            b.add(*args)
    assert b.size == 0 and b.has_returns is None
    # returns for some add() calls and not for others
    with pytest.raises(ValueError, match="returns were not given by the earlier add"):
        host_buffer(size=7, has_returns=False).add(f, meas, a, np.zeros(n))
    with pytest.raises(ValueError, match="returns were given by the earlier add"):
        host_buffer(size=7, has_returns=True).add(f, meas, a, None)
    with pytest.raises(ValueError, match="7 rows on top of 14 exceed the capacity of 20"):
        host_buffer(size=14, has_returns=False).add(f, meas, a, None)


def test_a_stacked_policy_and_bad_sizes_are_refused_by_name():
    from rollout import DemonstrationBuffer
    for k in (2, 0, True, "1", 1.0):
        with pytest.raises(ValueError, match="DemonstrationBuffer: latent stacking is not supported"):
            DemonstrationBuffer.stacked(_NoDevice(), _NoDevice(), 20, k)
    for kw in (dict(capacity=0), dict(capacity=True), dict(capacity=20, chunk=0), dict(capacity=20, chunk=1025), dict(capacity=2.5)):
        with pytest.raises(ValueError, match="DemonstrationBuffer: (capacity|chunk) is an int"):
            DemonstrationBuffer(_NoDevice(), _NoDevice(), **kw)


def test_clone_refuses_more_than_one_rank_with_the_buffers_message(monkeypatch):
    from mi355 import dist as midist
    monkeypatch.setattr(midist, "world_size", lambda: 2)
    with pytest.raises(ValueError, match=r"DemonstrationBuffer.clone: single rank only \(ragged rows give ranks different numbers of gradient all-reduces\)"):
        host_buffer(size=7, has_returns=False).clone()
