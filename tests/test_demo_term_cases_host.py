"""The problems of tests/demo_term_cases.py, checked on the CPU: every case is well conditioned (no sample exempted), the float64 reference at c_d = 0 is the PPO
reference, it is linear in c_d, and the host-side validation of the new settings refuses what it should -- none of which needs a GPU."""
import numpy as np
import pytest

import demo_term_cases as dc

GRID = [(s, mp, md) for s in ("A2", "A3") for mp, md in dc.COUNTS] + [("W", 33, 7)]


@pytest.mark.parametrize("shape,Mp,Md", GRID)
def test_every_case_is_well_conditioned(shape, Mp, Md):
    c = dc.case(shape, Mp, Md)
    cond = dc.conditioned(c)
    assert all(cond.values()), (shape, Mp, Md, cond)
    assert c.s.shape == (Mp, dc.SHAPES[shape][0]) and c.ds.shape == (Md, dc.SHAPES[shape][0]) and c.da.shape == (Md, dc.SHAPES[shape][1])
    assert (c.da >= c.low).all() and (c.da <= c.high).all() and np.isfinite(c.da).all()


@pytest.mark.parametrize("variant", list(dc.VARIANTS))
@pytest.mark.parametrize("kind", dc.KINDS)
@pytest.mark.parametrize("shape,Mp,Md", [("A3", 5, 3), ("A3", 33, 7), ("A2", 5, 3)])
def test_reference_at_zero_is_ppo_and_is_linear_in_the_coefficient(shape, Mp, Md, kind, variant):
    c = dc.case(shape, Mp, Md)
    vclip, kl = dc.VARIANTS[variant]
    ppo = dc.reference(c, 0.0, kind, vclip, kl, demo=False)
    r0, r1, r2 = (dc.reference(c, cd, kind, vclip, kl) for cd in (0.0, 0.5, 2.0))       # (0.5 and 2.0 are exact in fp32)
    assert r0["scal"]["loss"] == ppo["scal"]["loss"] == ppo["scal"]["ppo_loss"]
    for k in dc.NAMES:
        assert np.array_equal(r0["grads"][k], ppo["grads"][k]), k
        # g(c_d) = g_ppo + c_d g_demo: the slope between 0 and 0.5 is the slope between 0 and 2
        slope_a, slope_b = (r1["grads"][k] - r0["grads"][k]) / 0.5, (r2["grads"][k] - r0["grads"][k]) / 2.0
        scale = max(np.abs(r2["grads"][k]).max(), 1e-30)
        assert np.abs(slope_a - slope_b).max() <= 1e-12 * scale, k
    for k in dc.NAMES[7:]:                                 # the value net sees nothing of the demonstrations
        assert np.array_equal(r2["grads"][k], ppo["grads"][k]), k
    assert r1["scal"]["demo_loss"] == r2["scal"]["demo_loss"] and r1["scal"]["demo_loss"] > 0
    assert r2["scal"]["loss"] == pytest.approx(ppo["scal"]["loss"] + 2.0 * r2["scal"]["demo_loss"], rel=1e-14)
    for k in ("policy_loss", "value_loss", "entropy_loss", "ratio_mean"):
        assert r2["scal"][k] == ppo["scal"][k]
    if kind == "mse":
        assert r2["scal"]["demo_loss"] == r2["scal"]["mean_sq_error"]


def test_the_draw_rule():
    rng, state = np.random.RandomState(3), [None, 0]
    rows = dc.demonstration_rows(rng, state, 11, 4, 5)
    twin = np.random.RandomState(3)
    p1, p2, p3 = twin.permutation(11), twin.permutation(11), twin.permutation(11)
    want = [p1[0:4], p1[4:8], p2[0:4], p2[4:8], p3[0:4]]   # 3 rows remain behind two minibatches of 4: a fresh permutation
    assert all(np.array_equal(a, b) for a, b in zip(rows, want))
    rows = dc.demonstration_rows(np.random.RandomState(3), [None, 0], 11, 32, 2)      # batch_size above the size: all 11 rows, a fresh permutation every step
    twin = np.random.RandomState(3)
    assert np.array_equal(rows[0], twin.permutation(11)) and np.array_equal(rows[1], twin.permutation(11))


def test_the_buffers_draw_is_the_restated_rule():
    from rollout import RolloutBuffer
    dm = {"batch_size": 4, "rng": np.random.RandomState(9), "perm": None, "cursor": 0}
    got = np.concatenate([RolloutBuffer.demonstration_rows_drawn(dm, 11, 3), RolloutBuffer.demonstration_rows_drawn(dm, 11, 4)])
    want = dc.demonstration_rows(np.random.RandomState(9), [None, 0], 11, 4, 7)
    assert got.dtype == np.int32 and got.shape == (7, 4) and all(np.array_equal(a, b) for a, b in zip(got, want))


def _ppo(tmp_path):
    from oracle import ppo_oracle as po
    from ppo import PPO
    return PPO(np.array([67]), po.ActionSpace(), model_dir=str(tmp_path), seed=1)


def test_set_demonstration_loss_validates_without_a_device(tmp_path):
    m = _ppo(tmp_path)
    assert m.demo_coef is None
    for bad in (True, "1", -0.5, float("nan"), float("inf"), [1.0]):
        with pytest.raises(ValueError, match="set_demonstration_loss"):
            m.set_demonstration_loss(bad)
    with pytest.raises(ValueError, match="set_demonstration_loss"):
        m.set_demonstration_loss(1.0, loss="huber")
    assert m.demo_coef is None
    m.set_demonstration_loss(0.25, "mse")
    assert (m.demo_coef, m.demo_kind) == (0.25, "mse")
    m.set_demonstration_loss(0)
    assert (m.demo_coef, m.demo_kind) == (0.0, "nll")
    m.set_demonstration_loss(None)
    assert m.demo_coef is None
    with pytest.raises(ValueError, match="the demonstration term is off"):
        m._demo_rows(*[None] * 14)
