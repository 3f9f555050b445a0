"""Whole collect -> update cycles of both rollout buffers with the three NEWER settings -- advantage recomputation (set_advantage_recomputation), V-trace (set_vtrace)
and the demonstration term (set_demonstrations) -- on top of the seven older ones, against the float64 trainer of tests/rollout_trainer_cases.py, which states the
refresh, the V-trace finish and the demonstration step from include/mi355_carla.h and the module docstring of rollout.py and calls nothing of rollout.py, ppo.py or
mi355/.  The buffer-level tests of those settings (host_loop, vt_host_loop, test_update_is_a_host_loop_of_demo_steps) issue the device calls rollout.py issues, in
its order: they cannot see a wrong order, table or row set.  This file can: which states a refresh values (normalised, stacked, under the moments before this update's
merge), which rewards it reads (the scaled ones), which values value clipping reads (the recorded ones), which raw advantages per-minibatch normalisation reads and
which returns the diagnostics read from epoch 2 on (the refreshed ones), where a KL stop ends the refreshes, what a truncated segment bootstraps from at a refresh
(final_values_now), which cache of log pi_old the weights and the steps read, which tables the result returns, which rows the value term and the KL penalty average
over with demonstrations on, which stream the demonstration rows come from and when the coefficient's decay takes effect.

Per case and cycle (the helpers of test_zzzzzzzzz_rollout_all_settings_gpu.py): collect on the device with injected noise and the scripted rewards / dones /
truncations, read the tables back (final_states and the demonstration buffer's tables among them), run the update under a fixed numpy seed, run the reference in
float64 and float32 on the tables, and hold every returned number, the tables and the parameters to rollout_trainer_cases.compare().  The refreshed tables' bounds
are derived there per entry (the value bound and the log pi bound through the finish's own recurrence: Trainer.finish_bounds); tests/test_rollout_trainer_cases_host.py
shows on the CPU that the fp32 twin meets every bound and that each of the sixteen mis-statements above is seen at 10 x a bound or more.  Cases: rollout_trainer_cases.spec();
measured distances: profiles/r41_rollout_newer_settings.md."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "carla-ppo_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rollout_trainer_cases as rc  # noqa: E402
import test_zzzzzzzzz_rollout_all_settings_gpu as ag  # noqa: E402  (helpers only: World, make_buffer(), collect(), run_case(), padded())
from rollout_gpu_common import SENTINEL, bitwise, flat_state  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return ag.World(tmp_path_factory.mktemp("newer_settings"))


def refresh_figures(name, figures):
    """Prints, per cycle, the refreshed quantities' distances in units of their derived bounds and what the conditions rest on; -> the device's results."""
    for cycle, (out, ref) in enumerate(figures):
        line = ["recomputed_epochs %d" % out["recomputed_epochs"]] if "recomputed_epochs" in out else []
        if "vtrace_rho_clip_fraction" in out:
            line.append("clip fractions rho %.3f c %.3f, weights in [%.3f, %.3f], margin %.2e" % (
                out["vtrace_rho_clip_fraction"], out["vtrace_c_clip_fraction"], np.nanmin(out["refreshed_importance_weights"]), np.nanmax(out["refreshed_importance_weights"]),
                ref["margins"]["vtrace"].min()))
        if "demo_coef" in out:
            line.append("demo coef %.3g -> %.3g, %d redraws inside the update" % (out["demo_coef"], out["demo_coef_next"], int(ref["margins"]["demo_redraws"].sum())))
        print("%s cycle %d: %s" % (name, cycle, "; ".join(line)))
    return [out for out, _ in figures]


def newer_rows(world, name):
    """The rows of compare() that the newer settings added or changed, per cycle: {quantity: distance / bound} (the worst of the steps for a per-step row; the
    exact rows, whose bound is 0, are left out: run_case has asserted them)."""
    keep = ("refreshed_", "demo_loss", "demo_mean_sq_error", "minibatch mean", "minibatch std")
    out = []
    for rows in world.full[name]:
        d = {}
        for q, err, bound in rows:
            if q.startswith(keep) and bound > 0:
                d[q.split("[")[0]] = max(d.get(q.split("[")[0], 0.0), float("%.3g" % (err / bound)))
        out.append(d)
    return out


@pytest.mark.parametrize("name", ["H", "H-gae", "I", "I-batch"])
def test_refreshes_under_every_older_setting(world, name):
    """H: case A's three chained cycles (live / live / frozen, k = 2) with a V-trace refresh before epochs 2 and 3; H-gae: the GAE refresh; I / I-batch: the continuous
    buffer (a truncation and a done, k = 4, ddof 1) with two bars that differ, per-segment and batch normalisation."""
    sp = rc.spec(name)
    outs = refresh_figures(name, ag.run_case(world, name))
    print(name, "newer rows (distance / bound):", newer_rows(world, name))
    for out in outs:
        assert out["recomputed_epochs"] == sp["epochs"] - 1
        assert ("refreshed_importance_weights" in out) == (sp["vtrace"] is not None) and ("refreshed_final_values" in out) == (sp["kind"] == "continuous")
        assert not np.array_equal(out["refreshed_returns"], out["returns"], equal_nan=True)
    if name in ("H", "I"):
        assert all(0.1 <= out[k] <= 0.9 for out in outs for k in ("vtrace_rho_clip_fraction", "vtrace_c_clip_fraction"))
    if sp["kind"] == "continuous":                                                   # the truncated segments bootstrapped from refreshed final values, not the recorded ones
        for out in outs:
            cut = ~np.isnan(out["final_values"])
            assert cut.sum() == 2 and np.array_equal(np.isnan(out["refreshed_final_values"]), ~cut) and (out["refreshed_final_values"][cut] != out["final_values"][cut]).all()


@pytest.mark.parametrize("name", ["J", "J-mse", "J-plain"])
def test_the_demonstration_term_under_every_older_setting(world, name):
    """J: the demonstration term (7 rows in minibatches of 3, decay 0.5, two cycles, "nll") with recomputation, V-trace and six older settings on, observation
    normalisation frozen from given statistics in both buffers; J-mse: one cycle with "mse"; J-plain: without recomputation and V-trace."""
    sp = rc.spec(name)
    outs = refresh_figures(name, ag.run_case(world, name))
    print(name, "newer rows (distance / bound):", newer_rows(world, name))
    assert outs[0]["demo_coef"] == sp["demo"]["coef"] and outs[0]["demo_coef_next"] == sp["demo"]["coef"] * sp["demo"]["decay"]
    if len(outs) > 1:
        assert outs[1]["demo_coef"] == outs[0]["demo_coef_next"] != outs[0]["demo_coef"]
    for out in outs:
        assert ("recomputed_epochs" in out) == (name != "J-plain") and len(out["demo_losses"]) == len(out["losses"]) == len(out["demo_rows"])
        assert out["observation_rms"]["count"] == rc.GIVEN_OBS_ROWS               # frozen: the given statistics


def test_the_kl_stop_ends_the_refreshes(world):
    """Case L: the stop fires behind epoch 2 of 3, so exactly one refresh ran, and the legacy numpy stream is left where two epochs leave it (run_case asserts the
    stream against the reference's)."""
    (out, ref), = ag.run_case(world, "L")
    refresh_figures("L", [(out, ref)])
    print("L newer rows (distance / bound):", newer_rows(world, "L"))
    assert out["epochs_run"] == 2 and out["stopped_early"] and out["recomputed_epochs"] == 1 and len(out["losses"]) == 2 * 4


def test_case_h_in_bf16x3(world):
    """Case M.  The fp32 mode's distances are case H's (run here if that test has not run)."""
    if "H" not in world.rows:
        ag.run_case(world, "H")
    figures = ag.run_case(world, "M", fp32_mode=world.rows["H"])
    print("M newer rows (distance / bound):", newer_rows(world, "M"))
    assert len(figures) == 3 and all(out["recomputed_epochs"] == 2 for out, _ in figures)


@pytest.mark.parametrize("name", rc.H_CASES)
def test_leave_one_older_setting_out(world, name):
    figures = ag.run_case(world, name)
    refresh_figures(name, figures)
    print(name, "newer rows (distance / bound):", newer_rows(world, name))
    assert all(("epochs" in out) == rc.spec(name)["diagnostics"] and out["recomputed_epochs"] == 2 for out, _ in figures)


def test_two_runs_of_case_h_are_bitwise_equal_and_write_nothing_behind_the_tables(world):
    """Case H's first update twice from the same tables and the same state: every number, the parameters and the Adam slots bitwise; 8 sentinels behind each table
    the update writes -- values_now and logp_now among them -- survive.  Case H has neither truncations nor demonstrations (it is stacked), so the same is done
    with case I for the continuous buffer's final_values_now and with case J for the demonstration tables, which an update only reads."""
    import torch

    def twice(name, attrs, extra=()):
        sp = rc.spec(name)
        buf, m = ag.make_buffer(world, sp)
        ag.collect(buf, sp, rc.script(sp, 0))
        pads = []
        n_rows, dev = buf.n_table_rows, buf.device
        fresh = dict(mean_old=torch.zeros(n_rows, sp["A"], device=dev), _minibatch_advantages=torch.zeros(n_rows, device=dev), values_now=torch.zeros(n_rows, device=dev),
                     logp_now=torch.zeros(n_rows, device=dev))
        for attr in attrs:
            t, pad = ag.padded(fresh[attr] if attr in fresh else getattr(buf, attr))
            setattr(buf, attr, t)
            pads.append(pad)
        for owner, attr in extra:
            t, pad = ag.padded(getattr(owner(buf), attr))
            setattr(owner(buf), attr, t)
            pads.append(pad)
        live = [m.dev.params, m.dev.adam_m, m.dev.adam_v, m.dev.params_old, buf._reward_scaling["state"], buf._reward_scaling["carry"]]
        live += [buf._obs_norm[k] for k in ("state", "mean32", "inv32")]
        saved = [t.clone() for t in live]
        host = (m.beta1_power, m.beta2_power, m.kl_penalty, m.train_step_counter)
        demo = None if sp["demo"] is None else buf.demonstration_state()
        kw = dict(normalize=sp["normalize"]) if sp["kind"] == "continuous" else {}

        def once():
            np.random.seed(ag.SEED)
            out = buf.update_with_diagnostics(rc.GAMMA, rc.LAM, num_epochs=sp["epochs"], batch_size=sp["batch"], **kw)
            return out, [t.clone() for t in flat_state(m)] + ag.moments(buf, sp)
        out1, state1 = once()
        for t, s in zip(live, saved):
            t.copy_(s)
        m.beta1_power, m.beta2_power, m.kl_penalty, m.train_step_counter = host
        if demo is not None:
            buf.load_demonstration_state(demo)
        out2, state2 = once()
        assert bitwise(state1, state2) and not bitwise(state1[0], saved[0]), name
        assert out1["losses"] == out2["losses"] and out1["epochs"] == out2["epochs"] and out1["kl"] == out2["kl"] and out1["recomputed_epochs"] == out2["recomputed_epochs"] == 2
        keys = ["returns", "advantages", "raw_advantages", "grad_norms", "clip_scales", "minibatch_adv_stats", "minibatch_advantages", "scaled_rewards", "refreshed_values",
                "refreshed_returns", "refreshed_advantages", "refreshed_raw_advantages", "refreshed_importance_weights"]
        keys += ["refreshed_final_values"] if sp["kind"] == "continuous" else []
        for k in keys:
            assert np.array_equal(out1[k], out2[k], equal_nan=True), (name, k)
        assert out1["vtrace_rho_clip_fraction"] == out2["vtrace_rho_clip_fraction"] and out1["vtrace_c_clip_fraction"] == out2["vtrace_c_clip_fraction"]
        if demo is not None:
            assert out1["demo_losses"] == out2["demo_losses"] and all(np.array_equal(a, b) for a, b in zip(out1["demo_rows"], out2["demo_rows"]))
        torch.cuda.synchronize()
        assert all(bool((p == SENTINEL).all()) for p in pads), name
        print("%s: two runs of %d steps bitwise, %d sentinels behind each of %d tables untouched" % (name, len(out1["losses"]), ag.PAD, len(pads)))
    twice("H", ("returns", "advantages", "logp_old", "mean_old", "_minibatch_advantages", "values_now", "logp_now"))
    twice("I", ("returns", "advantages", "values_now", "logp_now", "final_values_now"))
    twice("J", ("returns", "advantages", "values_now", "logp_now"), extra=((lambda b: b._demo["buffer"], "states"), (lambda b: b._demo["buffer"], "expert_actions")))
