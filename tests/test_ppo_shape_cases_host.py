"""The problems of tests/ppo_shape_cases.py, on the host: every case the GPU tests use meets the clipped-branch conditions in float64 (10 % .. 60 % of the
samples on the zero-slope branch, both sides present, no ratio within 1e-3 of a clip edge, every ratio inside [1 / 20, 20]), and the same oracle run in float32 on
the CPU is inside the tolerances the GPU tests hold the kernels to -- so those tolerances are reachable in fp32 at these shapes."""
import numpy as np
import pytest
import torch

import ppo_shape_cases as pc


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def test_tables_name_the_cases_of_the_issue():
    shapes = {(v[0], v[1], v[2]): [] for v in pc.ENGINE_CASES.values()}
    for v in pc.ENGINE_CASES.values():
        shapes[(v[0], v[1], v[2])].append(v[3])
    assert shapes == {(67, 1, (500, 300)): [33, 77], (67, 3, (500, 300)): [33, 77, 300], (67, 8, (500, 300)): [33, 77],
                      (5, 3, (36, 20)): [33, 77], (96, 3, (132, 320)): [33, 77], (40, 3, (100, 44)): [33, 77],
                      (100, 3, (64, 64)): [5, 77], (67, 3, (64, 324)): [5, 77]}
    assert list(pc.HEAD_CASES) == [(A, M) for A in (1, 2, 3, 8) for M in (1, 255, 256, 257, 300)]
    assert len(pc.FUSED_CASES) == 13 and len(pc.PER_LAYER_CASES) == 4


@pytest.mark.parametrize("name", list(pc.ENGINE_CASES))
def test_engine_case_conditions_and_float32_oracle(name):
    c = pc.engine_case(name)
    print("\n%s: %s" % (name, c.cond))
    assert pc.conditions_met(c.cond), c.cond
    # the inputs are what the builder promises: actions inside the bounds, a logstd per action, bounds per action
    assert (c.a >= c.low).all() and (c.a <= c.high).all()
    assert len(set(c.theta_old["policy/action_logstd"].tolist())) == c.A and len(set(zip(c.low.tolist(), c.high.tolist()))) == c.A
    assert not any(lo == -1 and hi == 1 for lo, hi in zip(c.low, c.high))
    # the branch a sample is on is the reference's in float32 as well, and the float32 oracle is inside the GPU tolerances
    scal, ratio, mean, value, grads = pc.losses_and_grads(c.theta, c.theta_old, c.s, c.a, c.R, c.adv, c.low, c.high, dtype=torch.float32)
    assert np.array_equal(ratio > 1 + pc.EPS, c.ratio > 1 + pc.EPS) and np.array_equal(ratio < 1 - pc.EPS, c.ratio < 1 - pc.EPS)
    for k in pc.LOSS_KEYS:
        assert scal[k] == pytest.approx(c.scal[k], rel=pc.LOSS_REL, abs=pc.LOSS_ABS), k
    worst = {k: rel_err(grads[k], c.grads[k]) for k in c.grads}
    print("  float32 oracle, worst gradient error / tensor max: %.2e (%s)" % (max(worst.values()), max(worst, key=worst.get)))
    assert max(worst.values()) <= pc.GRAD_REL, worst
    assert all(np.abs(c.grads[k]).max() > 0 for k in c.grads)                     # no tensor's bound is relative to nothing
    assert np.allclose(mean, c.mean, rtol=pc.ACT_RTOL, atol=pc.ACT_ATOL) and np.allclose(value, c.value, rtol=pc.ACT_RTOL, atol=pc.ACT_ATOL)
    lp32 = pc.log_prob(c.theta_old, c.s, c.a, c.low, c.high, dtype=torch.float32)
    assert np.allclose(lp32, c.logp_old, rtol=pc.ACT_RTOL, atol=pc.ACT_ATOL)


@pytest.mark.parametrize("shape", sorted({(v[0], v[1], v[2]) for v in pc.ENGINE_CASES.values()}))
def test_predict_inputs_clamp_every_action_on_both_sides(shape):
    name = next(k for k, v in pc.ENGINE_CASES.items() if (v[0], v[1], v[2]) == shape)
    c = pc.engine_case(name)
    for M in (1, 8, 9, 33):
        p = pc.predict_inputs(c, M)
        if M >= 8:
            assert p["sides"]["low"].all() and p["sides"]["high"].all() and p["sides"]["inside"], (M, p["sides"])
        else:                                                                    # one row: every action is clamped, even indices at `high`, odd ones at `low`
            assert (p["sides"]["low"] | p["sides"]["high"]).all() and p["sides"]["high"][0] and (c.A < 2 or p["sides"]["low"][1])
        assert ((p["sampled"] == c.low) | (p["sampled"] == c.high)).any() and np.abs(p["sampled"] - p["mean"]).max() > 0.1


@pytest.mark.parametrize("A,M", list(pc.HEAD_CASES))
def test_head_case_conditions_and_float32_formulas(A, M):
    c = pc.head_case(A, M)
    print("\nA = %d, M = %d: %s" % (A, M, c.cond))
    assert pc.conditions_met(c.cond, single=M == 1), c.cond
    assert (c.act >= c.low).all() and (c.act <= c.high).all()
    r32 = pc.head_reference(c, torch.float32)
    assert np.array_equal(r32["ratio"] > 1 + pc.EPS, c.ratio > 1 + pc.EPS) and np.array_equal(r32["ratio"] < 1 - pc.EPS, c.ratio < 1 - pc.EPS)
    assert np.allclose(r32["losses"], c.losses, rtol=2e-5, atol=1e-6)              # the bounds of tests/test_ops_gpu.py
    assert np.allclose(r32["du"], c.du, rtol=2e-4, atol=1e-6) and np.allclose(r32["dv"], c.dv, rtol=1e-5, atol=1e-7) and np.allclose(r32["dls"], c.dls, rtol=2e-4, atol=1e-6)
    if M >= 4:
        assert c.sides["low"].all() and c.sides["high"].all() and c.sides["inside"], c.sides
    else:
        assert (c.sides["low"] | c.sides["high"]).all()
