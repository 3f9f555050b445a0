"""Host side of the adaptive KL penalty (no GPU): validators and the environment knob, the adaptation rule, kl_stats_summary, the state round trip, the C ABI's
names, and that state_dict() is what it was."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

import kl_penalty_cases as kc
from oracle import ppo_oracle as po

NEW_NAMES = ("mi_ppo_old_policy_cache", "mi_ppo_train_step_kl", "mi_ppo_kl_stats_scratch_doubles", "mi_ppo_kl_stats_idx")
BAD_COEF = (True, False, "0.5", float("nan"), float("inf"), -0.1, -0.0 - 1e-30, [0.5], np.float32("nan"))
BAD_TARGET = (True, "0.01", float("nan"), float("inf"), 0, 0.0, -0.01, [0.01])


def make(tmp_path, **kw):
    from ppo import PPO
    return PPO(np.array([67]), po.ActionSpace(), model_dir=str(tmp_path), seed=1, **kw)


def test_validators():
    from mi355.lib import kl_penalty_value, kl_target_value
    assert kl_penalty_value(None) is None and kl_penalty_value(0) == 0.0 and kl_penalty_value(np.float32(0.5)) == 0.5 and kl_penalty_value(3) == 3.0
    assert isinstance(kl_penalty_value(np.float64(0.25)), float)
    for bad in BAD_COEF:
        with pytest.raises(ValueError, match="who: the value is None or a finite float >= 0"):
            kl_penalty_value(bad, "who")
    assert kl_target_value(None) is None and kl_target_value(0.01) == 0.01
    for bad in BAD_TARGET:
        with pytest.raises(ValueError, match="who: the value is None"):
            kl_target_value(bad, "who")


def test_setter_before_a_device_exists(tmp_path, monkeypatch):
    monkeypatch.delenv("MI355_PPO_KL_COEF", raising=False)
    m = make(tmp_path)
    assert m.kl_penalty is None and m.kl_target is None and m.dev is None
    m.set_kl_penalty(0.5)
    assert (m.kl_penalty, m.kl_target) == (0.5, None)
    m.set_kl_penalty(0.2, target=0.01)
    assert (m.kl_penalty, m.kl_target) == (0.2, 0.01)
    for bad in BAD_COEF:
        with pytest.raises(ValueError, match="set_kl_penalty"):
            m.set_kl_penalty(bad)
    for bad in BAD_TARGET:
        with pytest.raises(ValueError, match="set_kl_penalty"):
            m.set_kl_penalty(0.2, target=bad)
    with pytest.raises(ValueError, match="target without a coefficient"):
        m.set_kl_penalty(None, target=0.01)
    assert (m.kl_penalty, m.kl_target) == (0.2, 0.01) and m.dev is None              # a refused call changes nothing and touches no device
    m.set_kl_penalty(0)
    assert m.kl_penalty == 0.0 and m.kl_target is None                               # 0 is on (measure only), and a call without a target drops the old one
    m.set_kl_penalty(None)
    assert m.kl_penalty is None and m.kl_target is None
    with pytest.raises(ValueError, match="is off"):
        m.adapt_kl_penalty(0.01)


def test_environment_knob(tmp_path, monkeypatch):
    for text, want in (("", None), ("  ", None), ("0", 0.0), ("0.5", 0.5), (" 2e-1 ", 0.2)):
        monkeypatch.setenv("MI355_PPO_KL_COEF", text)
        m = make(tmp_path)
        assert m.kl_penalty == want and m.kl_target is None
    for text in ("-1", "nan", "inf", "abc", "1,0"):
        monkeypatch.setenv("MI355_PPO_KL_COEF", text)
        with pytest.raises(ValueError, match="MI355_PPO_KL_COEF=%r: expected a finite float >= 0" % text):
            make(tmp_path)
    monkeypatch.delenv("MI355_PPO_KL_COEF")
    assert make(tmp_path).kl_penalty is None


# (kl, target, beta) -> beta': both thresholds themselves change nothing (the comparisons are strict)
T = 0.01
RULE = [
    (0.0, T, 0.5, 0.25), (T / 1.5 * 0.999, T, 0.5, 0.25), (T / 1.5, T, 0.5, 0.5), (T, T, 0.5, 0.5), (1.5 * T, T, 0.5, 0.5), (1.5 * T * 1.001, T, 0.5, 1.0),
    (1.0, T, 0.5, 1.0), (0.0, None, 0.5, 0.5), (1.0, None, 0.5, 0.5), (0.0, T, 0.0, 0.0), (1.0, T, 0.0, 0.0), (0.02, 0.02, 3.0, 3.0), (0.2, 0.02, 3.0, 6.0),
]


@pytest.mark.parametrize("kl,target,beta,want", RULE)
def test_adaptation_rule(tmp_path, kl, target, beta, want):
    from ppo import adapted_kl_coef
    assert adapted_kl_coef(beta, target, kl) == want == kc.adapted(beta, target, kl)
    m = make(tmp_path)
    m.set_kl_penalty(beta, target)
    assert m.adapt_kl_penalty(kl) == want and m.kl_penalty == want and m.kl_target == target
    assert m.adapt_kl_penalty(np.float64(kl)) == kc.adapted(want, target, kl)       # numpy scalars are taken; the rule applies again


@pytest.mark.parametrize("target", [None, 0.01])
def test_adaptation_refuses_a_kl_that_is_no_kl(tmp_path, target):
    m = make(tmp_path)
    m.set_kl_penalty(0.5, target)
    for bad in (float("nan"), float("inf"), -float("inf"), -1e-9, "0.01", None, True):
        with pytest.raises(ValueError, match="adapt_kl_penalty"):
            m.adapt_kl_penalty(bad)
        assert m.kl_penalty == 0.5 and m.kl_target == target


def test_kl_stats_summary_against_numpy():
    from mi355.ppo_device import N_KL_STATS, kl_stats_summary
    assert N_KL_STATS == 4
    rng = np.random.RandomState(5)
    kl, part = rng.uniform(0.0, 0.4, 1000), rng.uniform(0.0, 0.1, 1000)
    s = kl_stats_summary([len(kl), kl.sum(), (kl * kl).sum(), part.sum()])
    assert set(s) == {"samples", "kl", "kl_std", "kl_mean_part"} and s["samples"] == 1000 and isinstance(s["samples"], int)
    assert s["kl"] == pytest.approx(kl.mean(), rel=1e-13) and s["kl_std"] == pytest.approx(kl.std(), rel=1e-10) and s["kl_mean_part"] == pytest.approx(part.mean(), rel=1e-13)
    assert all(isinstance(s[k], float) for k in ("kl", "kl_std", "kl_mean_part"))
    one = kl_stats_summary(np.array([1.0, 0.25, 0.0625, 0.1]))
    assert one == {"samples": 1, "kl": 0.25, "kl_std": 0.0, "kl_mean_part": 0.1}
    assert kl_stats_summary([3.0, 0.0, 0.0, 0.0])["kl_std"] == 0.0                   # a variance that rounds below zero is clamped, not NaN
    assert kl_stats_summary([2.0, 0.2, 0.02 * (1 - 1e-16), 0.0])["kl_std"] == 0.0
    assert math.isnan(kl_stats_summary([2.0, float("nan"), 0.0, 0.0])["kl"])
    for bad in ([1.0, 2.0, 3.0], np.zeros(5), [0.0, 0.0, 0.0, 0.0], [-1.0, 0.0, 0.0, 0.0]):
        with pytest.raises(ValueError, match="kl_stats_summary"):
            kl_stats_summary(bad)


def test_state_round_trip(tmp_path):
    a, b = make(tmp_path / "a"), make(tmp_path / "b")
    assert a.kl_penalty_state() == {"kl_coef": None, "kl_target": None}
    a.set_kl_penalty(0.3, 0.02)
    a.adapt_kl_penalty(1.0)
    st = a.kl_penalty_state()
    assert st == {"kl_coef": 0.6, "kl_target": 0.02}
    b.load_kl_penalty_state(st)
    assert b.kl_penalty_state() == st and b.adapt_kl_penalty(0.0) == a.adapt_kl_penalty(0.0) == 0.3
    b.load_kl_penalty_state({"kl_coef": None, "kl_target": None})
    assert b.kl_penalty is None
    for bad in ({}, {"kl_coef": 0.1}, {"kl_coef": 0.1, "kl_target": None, "more": 1}):
        with pytest.raises(ValueError, match="load_kl_penalty_state"):
            a.load_kl_penalty_state(bad)
    with pytest.raises(ValueError, match="set_kl_penalty"):
        a.load_kl_penalty_state({"kl_coef": -1.0, "kl_target": None})
    assert a.kl_penalty_state() == {"kl_coef": 0.3, "kl_target": 0.02}


def test_the_c_abi_has_the_new_names():
    from mi355 import lib as milib
    protos = milib.parse_header()
    cdll = ctypes.CDLL(milib.LIB_PATH)
    for name in NEW_NAMES:
        assert name in protos, name
        assert getattr(cdll, name) is not None
    assert [t for t, _ in protos["mi_ppo_old_policy_cache"][1]] == ["void*", "void*", "const float*", "const float*", "int", "float*", "float*"]
    assert [n for _, n in protos["mi_ppo_train_step_kl"][1]] == ["h", "comm", "stream", "states", "actions", "returns", "advantage", "logp_old", "mean_old", "kl_coef",
                                                                  "old_values", "clip_range_vf", "row_idx", "n_rows", "M", "inv_m", "grad_scale", "adam", "alpha", "beta1",
                                                                  "beta2", "epsilon"]
    assert protos["mi_ppo_kl_stats_scratch_doubles"] == ("long long", [("int", "M")])
    assert [n for _, n in protos["mi_ppo_kl_stats_idx"][1]] == ["h", "stream", "states", "mean_old", "row_idx", "n_rows", "M", "accumulate", "scratch", "stats"]
    text = open(milib.HEADER).read()
    assert "#define MI_PPO_N_KL_STATS 4" in text and "KL(pi_old || pi_theta)" in text
    # the scratch size needs no device: a row of MI_PPO_N_KL_STATS doubles per block of 32 samples
    cdll.mi_ppo_kl_stats_scratch_doubles.restype = ctypes.c_longlong
    assert [cdll.mi_ppo_kl_stats_scratch_doubles(m) for m in (0, 1, 32, 33, 4096)] == [4, 4, 4, 8, 512]
    # a null handle is refused before anything else is looked at
    cdll.mi_last_error.restype = ctypes.c_char_p
    for name in ("mi_ppo_old_policy_cache", "mi_ppo_train_step_kl", "mi_ppo_kl_stats_idx"):
        fn = getattr(cdll, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [milib._CTYPES[t] for t, _ in protos[name][1]]
        args = [None if t is ctypes.c_void_p else 1 for t in fn.argtypes]
        assert fn(*args) == -4 and name.encode() + b": null handle" in cdll.mi_last_error(), name      # MI_ERR_STATE


def test_state_dict_is_untouched():
    from ppo import PPO
    src = inspect.getsource(PPO.state_dict) + inspect.getsource(PPO.load_state_dict)
    assert "kl" not in src.lower()
    import rollout
    for cls in (rollout.RolloutBuffer, rollout.ContinuousRolloutBuffer):
        assert "set_kl_penalty" not in dir(cls)                                      # the buffers read ppo.kl_penalty: no setter of their own


def test_the_reference_is_well_conditioned_at_every_shape():
    """The float64 figures the GPU tests lean on, for all six (shape, M) pairs: mean KL >= 0.1, the fp32 floor <= 1e-4 of it, no negative KL[m]."""
    for shape in kc.SHAPES:
        for M in kc.MS:
            c, ref = kc.case(shape, M)
            s = ref["scal"]
            print("%s M = %d: mean KL %.6f, floor / KL %.2e, penalty %.6f" % (shape, M, s["kl"], s["floor"] / s["kl"], s["penalty"]))
            assert kc.well_conditioned(ref)
            assert s["penalty"] == pytest.approx(kc.BETA32 * s["kl"], rel=1e-15) and s["bound"] <= 2.0 * kc.KL_REL * s["kl"]
            assert np.array_equal(c.theta["policy/action_logstd"], (c.theta_old["policy/action_logstd"] + kc.logstd_shift(c.A)).astype(np.float32))
            # the spelling without the cancellation agrees with the textbook one
            sig2, sigo2 = np.exp(2.0 * c.theta["policy/action_logstd"].astype(np.float64)), np.exp(2.0 * c.theta_old["policy/action_logstd"].astype(np.float64))
            D = ref["mean"] - kc.old_means(c)
            textbook = (0.5 * np.log(sig2 / sigo2) + (sigo2 + D * D) / (2.0 * sig2) - 0.5).sum(-1)
            assert np.allclose(textbook, ref["kl_m"], rtol=1e-10, atol=1e-14)
