"""CPU-only tests of dual-clip PPO and the runtime loss coefficients (mi_ppo_set_dual_clip / mi_ppo_dual_clip, mi_ppo_set_loss_coefs / mi_ppo_loss_coefs,
mi_ppo_dual_clip_stats, PPO.set_dual_clip, PPO.set_loss_coefficients, MI355_PPO_DUAL_CLIP): the planned cases of tests/dual_clip_cases.py meet their three
conditions on the reference alone, the float64 reference agrees with finite differences, the C-ABI surface and every argument error the host can reach without
an engine, the setters' validation on an object without a session, the environment knob, the refusal texts and dual_clip_summary's arithmetic."""
import ctypes
import inspect
import math
import os
import types

import numpy as np
import pytest

import dual_clip_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = "const float*"
STATS_PROTO = ("int", [("void*", "stream"), (F, "logp_new"), (F, "logp_old"), (F, "advantage"), ("const int*", "row_idx"), ("int", "n_rows"), ("int", "M"),
                       ("float", "clip_eps"), ("float", "dual_clip"), ("int", "accumulate"), ("double*", "scratch"), ("double*", "stats")])


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("shape,M", [(s, M) for s in dc.SHAPES for M in dc.MS])
def test_the_planned_rows_meet_their_conditions(shape, M, positive):
    q = dc.planned(shape, M, positive)
    cond = dc.plan_conditions(q)
    print("\n%s M = %d%s: classes %s, smallest distance from a threshold %.4f of it, smallest |A| %.3f"
          % (shape, M, " (A > 0)" if positive else "", [dc.CLASS_NAMES[k] for k in cond["present"]], cond["gap"], cond["a_min"]))
    assert cond["gap"] >= dc.MARGIN and cond["a_min"] >= dc.A_MIN
    assert np.allclose(q.ratio, q.target, rtol=1e-6, atol=0)                         # the fp32 cache realises the targets
    if positive:
        assert np.all(q.adv > 0) and dc.DUAL not in cond["present"] and not dc.reference(q.theta, q.s, q.a, q.R, q.adv, q.logp_old, q.low, q.high, grads=False)[2]["dual"].any()
        return
    assert cond["present"] == dc.expected_classes(M)
    # the plan's class of every row is the definition's, and the counts are the plan's
    want = np.array([dc.class_of(t, s) for t, s in dc.PLAN])[np.arange(M) % len(dc.PLAN)]
    assert np.array_equal(q.cls, want)
    per = dc.reference(q.theta, q.s, q.a, q.R, q.adv, q.logp_old, q.low, q.high, grads=False)[2]
    assert np.array_equal(per["dual"], q.cls == dc.DUAL)
    assert np.all(per["du"][q.cls == dc.DUAL] == 0.0) and np.all(per["du"][(q.cls == dc.NEG_LOW) | (q.cls == dc.POS_HIGH)] == 0.0)
    flowing = (q.cls == dc.NEG_FLOW) | (q.cls == dc.POS_LOW) | (q.cls == dc.POS_IN)
    assert np.all(np.abs(per["du"][flowing]).max(axis=1) > 0.0)
    assert np.all(per["surrogate_dual"][per["dual"]] > per["surrogate"][per["dual"]]) and np.array_equal(per["surrogate_dual"][~per["dual"]], per["surrogate"][~per["dual"]])


def test_c_infinite_is_the_plain_loss_and_matches_the_oracle():
    """reference() with c = inf against oracle.ppo_oracle.ppo_losses (float64 autograd) on the log pi_old that theta_old gives: two independent spellings."""
    import ppo_shape_cases as pc
    c = pc.build(5, 3, (36, 20), 33, 11, 0.0231)
    scal, g, per = dc.reference(c.theta, c.s, c.a, c.R, c.adv, c.logp_old, c.low, c.high, c=float("inf"), eps=pc.EPS)
    assert not per["dual"].any()
    for k in pc.LOSS_KEYS:
        assert scal[k] == pytest.approx(c.scal[k], rel=1e-11, abs=1e-13), k
    for k in dc.NAMES:
        assert np.abs(g[k] - c.grads[k]).max() <= 1e-11 * max(np.abs(c.grads[k]).max(), 1e-30), k


def test_the_reference_against_finite_differences():
    """Every element of the 13 variables of the 5 -> 36 / 20 policy at M = 5, central differences of the float64 loss with h = 1e-6: the loss is piecewise smooth,
    the samples are away from the ReLU kinks (ppo_shape_cases.near_relu_kink) and the rows 8 % and more from the ratio's thresholds."""
    q = dc.planned("A3", 5)
    theta = {k: np.asarray(v, np.float64) for k, v in q.theta.items()}
    loss = lambda th: dc.reference(th, q.s, q.a, q.R, q.adv, q.logp_old, q.low, q.high, grads=False)[0]["loss"]      # noqa: E731
    _, g, per = dc.reference(theta, q.s, q.a, q.R, q.adv, q.logp_old, q.low, q.high)
    assert per["dual"].sum() == 1
    h, worst = 1e-6, {}
    for k in dc.NAMES:
        fd = np.zeros(theta[k].size)
        flat = theta[k].reshape(-1)
        for i in range(flat.size):
            keep = flat[i]
            flat[i] = keep + h
            up = loss(theta)
            flat[i] = keep - h
            dn = loss(theta)
            flat[i] = keep
            fd[i] = (up - dn) / (2 * h)
        worst[k] = float(np.abs(fd - g[k].reshape(-1)).max() / max(np.abs(g[k]).max(), 1e-30))
    print("\nfinite differences, worst distance per tensor as a share of its max: %s" % {k: "%.2e" % v for k, v in worst.items()})
    # (central differences at h = 1e-6 in float64: truncation ~h^2, rounding ~1e-16 / h = 1e-10 of the loss's scale)
    assert not {k: v for k, v in worst.items() if v > 1e-6}


def test_entry_points_are_declared_and_exported():
    from mi355 import lib as milib
    from mi355 import ppo_device
    protos = milib.parse_header()
    assert protos["mi_ppo_set_dual_clip"] == ("int", [("void*", "h"), ("float", "c")])
    assert protos["mi_ppo_dual_clip"] == ("float", [("void*", "h")])
    assert protos["mi_ppo_set_loss_coefs"] == ("int", [("void*", "h"), ("float", "clip_eps"), ("float", "value_scale"), ("float", "entropy_scale")])
    assert protos["mi_ppo_loss_coefs"] == ("int", [("void*", "h"), ("float*", "clip_eps"), ("float*", "value_scale"), ("float*", "entropy_scale")])
    assert protos["mi_ppo_dual_clip_stats_scratch_doubles"] == ("long long", [("int", "M")])
    assert protos["mi_ppo_dual_clip_stats"] == STATS_PROTO
    L = milib.get()
    for name in ("mi_ppo_set_dual_clip", "mi_ppo_dual_clip", "mi_ppo_set_loss_coefs", "mi_ppo_loss_coefs", "mi_ppo_dual_clip_stats_scratch_doubles", "mi_ppo_dual_clip_stats"):
        assert hasattr(L.cdll, name), name
    assert L.mi_abi_version() == 7                                                   # entries added, none changed
    text = open(milib.HEADER).read()
    assert "#define MI_PPO_N_DUAL_CLIP_STATS 5" in text and ppo_device.N_DUAL_CLIP_STATS == 5
    i = text.index("int mi_ppo_set_dual_clip")
    comment = text[text.rfind("/*", 0, i):i]
    for c in ("s' = (A < 0 && c A > s) ? c A : s", "tf.maximum", "exactly 0.0", "-0.0 included", "c = +inf", "every stored bit", "mi_ppo_clone_step", "MI_ERR_SHAPE",
              "mi_ppo_set_max_grad_norm", "mi_ppo_update_stats_idx", "no atomics", "not read", "__expf(lp - lp_old)"):
        assert c in comment, c
    sd = L.mi_ppo_dual_clip_stats_scratch_doubles
    assert [sd(m) for m in (-3, 0, 1, 256, 257, 4096)] == [5, 5, 5, 5, 10, 80]


def test_every_host_checkable_argument_error():
    from mi355 import lib as milib
    L = milib.get()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    err, f = L.cdll.mi_last_error, ctypes.c_float
    L.cdll.mi_ppo_dual_clip.restype = ctypes.c_float
    assert L.cdll.mi_ppo_set_dual_clip(None, f(3.0)) == -4 and err() == b"mi_ppo_set_dual_clip: null handle"
    assert L.cdll.mi_ppo_set_dual_clip(None, f(-1.0)) == -4                            # the handle first
    assert L.cdll.mi_ppo_dual_clip(None) == -1.0 and err() == b"mi_ppo_dual_clip: null handle"
    assert L.cdll.mi_ppo_set_loss_coefs(None, f(0.2), f(1.0), f(0.0)) == -4 and err() == b"mi_ppo_set_loss_coefs: null handle"
    assert L.cdll.mi_ppo_loss_coefs(None, p, p, p) == -4 and err() == b"mi_ppo_loss_coefs: null handle"
    with pytest.raises(milib.MiError, match="mi_ppo_set_dual_clip failed"):
        L.mi_ppo_set_dual_clip(None, 3.0)
    stats = L.cdll.mi_ppo_dual_clip_stats

    def scall(lp=p, lpo=p, adv=p, rows=p, n_rows=8, M=5, eps=0.2, c=3.0, acc=0, scratch=p, out=p):
        return stats(None, lp, lpo, adv, rows, n_rows, M, f(eps), f(c), acc, scratch, out)
    for kw in (dict(M=0), dict(M=-2), dict(n_rows=0)):
        assert scall(**kw) == -1 and err().startswith(b"mi_ppo_dual_clip_stats: empty input"), kw
    for name in ("lp", "lpo", "adv", "rows", "scratch", "out"):
        assert scall(**{name: None}) == -1 and err().startswith(b"mi_ppo_dual_clip_stats: missing buffers"), name
    for bad in (0.0, -0.2, float("inf"), float("nan")):
        assert scall(eps=bad) == -1 and err().startswith(b"mi_ppo_dual_clip_stats: clip_eps"), bad
    for bad in (0.0, 1.0, 0.5, -3.0, float("nan"), float("-inf")):
        assert scall(c=bad) == -1 and err().startswith(b"mi_ppo_dual_clip_stats: dual_clip"), bad
    for bad in (-1, 2):
        assert scall(acc=bad) == -1 and err().startswith(b"mi_ppo_dual_clip_stats: accumulate"), bad
    assert scall(c=float("inf"), acc=3) == -1 and err().startswith(b"mi_ppo_dual_clip_stats: accumulate")      # +inf is a valid constant: the next check answers
    assert all(x == 0.0 for x in buf)                                                  # the dummy buffers were not written


class _Space:
    shape = (2,)
    low = np.array([-1.0, 0.0], np.float32)
    high = np.array([1.0, 1.0], np.float32)


def make_ppo(tmp_path, **kw):
    from ppo import PPO
    return PPO(np.array([67]), _Space(), model_dir=str(tmp_path), **kw)


BAD_C = (0, 0.0, 1, 1.0, 0.5, -3.0, float("nan"), -float("inf"), True, False, "3", [3.0])


def test_set_dual_clip_validation_without_a_session(tmp_path, monkeypatch):
    monkeypatch.delenv("MI355_PPO_DUAL_CLIP", raising=False)
    m = make_ppo(tmp_path)
    assert m.dual_clip is None and m.dev is None
    for good, want in ((3, 3.0), (1.5, 1.5), (np.float32(2.5), 2.5), (float("inf"), float("inf")), (None, None)):
        m.set_dual_clip(good)
        assert m.dual_clip == want and (want is None or isinstance(m.dual_clip, float))
    m.set_dual_clip(3.0)
    for bad in BAD_C:
        with pytest.raises(ValueError, match=r"PPO\.set_dual_clip: the value is None or a float > 1"):
            m.set_dual_clip(bad)
        assert m.dual_clip == 3.0 and m.dev is None, bad                               # refused before anything changed or touched a device
    assert "dual_clip" not in inspect.getsource(type(m).state_dict) and "dual_clip" not in inspect.getsource(type(m).load_state_dict)


def test_the_environment_knob(tmp_path, monkeypatch):
    for text, want in (("3", 3.0), (" 1.5 ", 1.5), ("inf", float("inf")), ("", None)):
        monkeypatch.setenv("MI355_PPO_DUAL_CLIP", text)
        assert make_ppo(tmp_path).dual_clip == want, text
    monkeypatch.delenv("MI355_PPO_DUAL_CLIP")
    assert make_ppo(tmp_path).dual_clip is None
    for text in ("0", "1", "0.5", "-3", "nan", "three", "-inf"):
        monkeypatch.setenv("MI355_PPO_DUAL_CLIP", text)
        with pytest.raises(ValueError, match="MI355_PPO_DUAL_CLIP"):
            make_ppo(tmp_path)
    monkeypatch.setenv("MI355_PPO_DUAL_CLIP", "3")                                    # set_dual_clip overrides what the knob supplied
    m = make_ppo(tmp_path)
    m.set_dual_clip(None)
    assert m.dual_clip is None
    assert "MI355_PPO_DUAL_CLIP" in open(os.path.join(ROOT, "DESIGN.md")).read()        # the Python-side knob table


def test_set_loss_coefficients_validation_without_a_session(tmp_path):
    m = make_ppo(tmp_path, epsilon=0.2, value_scale=0.5, entropy_scale=0.01)
    m.set_loss_coefficients()
    assert (m.epsilon, m.value_scale, m.entropy_scale) == (0.2, 0.5, 0.01)
    m.set_loss_coefficients(epsilon=0.1)
    assert (m.epsilon, m.value_scale, m.entropy_scale) == (0.1, 0.5, 0.01)
    m.set_loss_coefficients(value_scale=0, entropy_scale=np.float32(0.0))
    assert (m.epsilon, m.value_scale, m.entropy_scale) == (0.1, 0.0, 0.0) and all(isinstance(x, float) for x in (m.epsilon, m.value_scale, m.entropy_scale))
    m.set_loss_coefficients(0.2, 1.0, 0.01)
    for kw, name in ((dict(epsilon=0), "clip_eps"), (dict(epsilon=-0.2), "clip_eps"), (dict(epsilon=float("inf")), "clip_eps"), (dict(epsilon=float("nan")), "clip_eps"),
                     (dict(epsilon=True), "clip_eps"), (dict(epsilon="0.2"), "clip_eps"), (dict(value_scale=-1.0), "value_scale"), (dict(value_scale=float("inf")), "value_scale"),
                     (dict(value_scale=float("nan")), "value_scale"), (dict(entropy_scale=-0.01), "entropy_scale"), (dict(entropy_scale=False), "entropy_scale"),
                     (dict(epsilon=0.1, entropy_scale=float("nan")), "entropy_scale")):
        with pytest.raises(ValueError, match=r"PPO\.set_loss_coefficients: %s is a finite float" % name):
            m.set_loss_coefficients(**kw)
        assert (m.epsilon, m.value_scale, m.entropy_scale) == (0.2, 1.0, 0.01) and m.dev is None, kw


def test_the_validation_functions():
    from mi355.lib import dual_clip_value, loss_coef_values
    assert dual_clip_value(None) is None and dual_clip_value(2) == 2.0 and math.isinf(dual_clip_value(float("inf")))
    for bad in BAD_C:
        with pytest.raises(ValueError, match="who: the value is None or a float > 1"):
            dual_clip_value(bad, "who")
    assert loss_coef_values(0.2, 0, 0.0) == (0.2, 0.0, 0.0)
    for bad in ((0, 1, 1), (0.2, -1, 0), (0.2, 1, float("inf")), (float("nan"), 1, 0), (True, 1, 0), ("0.2", 1, 0)):
        with pytest.raises(ValueError, match="who: .* is a finite float"):
            loss_coef_values(*bad, who="who")


class _StubDev:
    def __init__(self, fused):
        self.fused, self.calls = fused, []

    def fused_ok(self):
        return self.fused

    def train_step(self, *a, **kw):
        self.calls.append("train_step")


def test_dispatch_refuses_the_per_layer_path(tmp_path, monkeypatch):
    monkeypatch.delenv("MI355_PPO_DUAL_CLIP", raising=False)
    monkeypatch.delenv("MI355_PPO_FUSED", raising=False)
    m = make_ppo(tmp_path)
    m.dev = _StubDev(False)
    m.dual_clip = 3.0
    text = (r"PPO: dual clip \(PPO\.set_dual_clip\) exists only in the fused kernels \(this policy's shape is outside their range \(more than 96 inputs: "
            r"PPO\.set_wide_inputs\(\)\) or MI355_PPO_FUSED=0\)")
    with pytest.raises(ValueError, match=text):
        m._dispatch_step(None, None, None, None, None, None, None, None, 4, 4)
    m.dev = _StubDev(True)
    monkeypatch.setenv("MI355_PPO_FUSED", "0")
    with pytest.raises(ValueError, match=text):
        m._dispatch_step(None, None, None, None, None, None, None, None, 4, 4)
    assert m.dev.calls == [] and m.beta1_power == np.float32(0.9)                     # nothing was called, Adam's powers did not advance
    monkeypatch.delenv("MI355_PPO_FUSED")
    m._dispatch_step(None, None, None, None, None, None, None, None, 4, 4)            # fused: the plain one-call step, which reads the handle's setting
    assert m.dev.calls == ["train_step"]
    m.dual_clip, m.dev = None, _StubDev(False)                                        # off: fused_ok() is not asked and the C entry falls back by itself
    m.dev.fused_ok = None
    m._dispatch_step(None, None, None, None, None, None, None, None, 4, 4)
    assert m.dev.calls == ["train_step"]
    m.dev = None


@pytest.mark.parametrize("name", ["RolloutBuffer", "ContinuousRolloutBuffer"])
def test_the_buffers_refuse_without_the_fused_kernels(name):
    import rollout
    cls = getattr(rollout, name)
    ppo = types.SimpleNamespace(dual_clip=3.0, _need_dev=lambda: _StubDev(False))
    fake = type(name, (), {})()                                                       # (the message starts with the buffer's class name)
    fake.ppo = ppo
    with pytest.raises(ValueError, match=name + r"\.update: dual clip \(PPO\.set_dual_clip\) exists only in the fused kernels \(this policy's shape is outside the "
                                                r"fused range \(more than 96 inputs: PPO\.set_wide_inputs\(\)\) or MI355_PPO_FUSED=0\)"):
        cls._check_update(fake, 1, 4, None, None)


def test_signatures_and_documents():
    import rollout
    from mi355.ppo_device import PpoDevice
    from ppo import PPO
    names = lambda fn: list(inspect.signature(fn).parameters)      # noqa: E731
    assert names(PPO.set_dual_clip) == ["self", "c"]
    assert names(PPO.set_loss_coefficients) == ["self", "epsilon", "value_scale", "entropy_scale"]
    assert all(p.default is None for k, p in inspect.signature(PPO.set_loss_coefficients).parameters.items() if k != "self")
    assert names(PpoDevice.set_dual_clip) == ["self", "c"] and names(PpoDevice.set_loss_coefs) == ["self", "clip_eps", "value_scale", "entropy_scale"]
    assert names(PpoDevice.dual_clip_stats) == ["self", "logp_new", "logp_old", "advantage", "row_idx", "M", "clip_eps", "dual_clip", "stats", "scratch", "accumulate"]
    assert names(PPO.train) == ["self", "input_states", "taken_actions", "returns", "advantage"] == names(PPO.train_step)      # no extra inputs
    for c in ("dual_clip_fraction", "negative_advantage_fraction", "surrogate_mean", "surrogate_mean_unclipped", "set_dual_clip"):
        assert c in rollout.RolloutBuffer.update_with_diagnostics.__doc__, c
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "test_zzzzzzzzzzzzzzzz_dual_clip_gpu.py" in readme and "set_dual_clip" in readme
    assert os.path.exists(os.path.join(ROOT, "profiles", "r42_dual_clip.md"))


def test_dual_clip_summary():
    from mi355.ppo_device import dual_clip_summary
    out = dual_clip_summary([8.0, 4.0, 2.0, -6.0, -10.0])
    assert out == {"dual_clip_fraction": 0.25, "negative_advantage_fraction": 0.5, "surrogate_mean": -0.75, "surrogate_mean_unclipped": -1.25}
    for bad in ([1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0], np.zeros(9)):
        with pytest.raises(ValueError, match="dual_clip_summary"):
            dual_clip_summary(bad)


def test_the_new_kernel_in_the_gfx950_listing():
    from rollout_host_common import _kernel, _listing
    fused = _listing("ppo_fused")
    name, body, scratch, lds = _kernel(fused, r"_ZN2mi26ppo_dual_clip_stats_kernelE")
    assert scratch == 0 and lds == 4 * 5 * 8, (name, scratch, lds)                    # five doubles per wave in the block reduction, nothing else
    assert "atomic" not in body and "v_add_f64" in body and "v_mul_f64" in body and "v_exp_f32" in body, name
