"""The float64 trainer of tests/rollout_trainer_cases.py on synthetic collections, no device: the cases meet the conditions their bounds rest on, the fp32 twin stays
inside the bounds the GPU tests (test_zzzzzzzzz_rollout_all_settings_gpu.py; for the cases of the newer settings -- advantage recomputation, V-trace, the
demonstration term -- test_zzzzzzzzzzzzzzz_rollout_newer_settings_gpu.py) assert, every mis-ordering the suite could not see is caught by those bounds at 10 x or
more, and the module stands apart from the code it checks."""
import ast
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rollout_trainer_cases as rc  # noqa: E402

CASES = ("A", "B", "C", "D", "F", "G", "K") + rc.E_CASES + rc.NEWER_CASES
REFRESH_KEYS = ("refreshed_values", "refreshed_returns", "refreshed_advantages", "refreshed_raw_advantages")
VTRACE_KEYS = ("refreshed_importance_weights", "vtrace_rho_clip_fraction", "vtrace_c_clip_fraction")
DEMO_KEYS = ("demo_losses", "demo_rows", "demo_coef", "demo_coef_next")
_RUNS = {}


def runs(name):
    """(float64 results, twin results, collections) of a case, computed once and not to be modified."""
    if name not in _RUNS:
        outs, _, cols = rc.run_host(name)
        twin, _, _ = rc.run_host(name, torch.float32, feed=cols)
        _RUNS[name] = (outs, twin, cols)
    return _RUNS[name]


@pytest.mark.parametrize("name", CASES)
def test_conditions_hold_on_the_reference(name):
    sp = rc.spec(name)
    outs, _, cols = runs(name)
    fig = rc.check_conditions(name, outs)
    print(name, fig)
    assert len(outs) == len(sp["cycles"])
    for o in outs:
        steps = -(-o["samples"] // sp["batch"])
        assert len(o["losses"]) == steps * (o["epochs_run"] if sp["diagnostics"] else sp["epochs"])
        assert np.isnan(o["raw_advantages"]).sum() == sp["E"] * sp["T"] - o["samples"]
    # ---- the newer settings: with a setting off its keys are absent, with it on every one is there
    for o in outs:
        assert ("recomputed_epochs" in o) == bool(sp["recompute"]) and all((k in o) == bool(sp["recompute"]) for k in REFRESH_KEYS), name
        assert all((k in o) == (sp["vtrace"] is not None) for k in VTRACE_KEYS) and all((k in o) == (sp["demo"] is not None) for k in DEMO_KEYS), name
        assert ("refreshed_final_values" in o) == (bool(sp["recompute"]) and sp["kind"] == "continuous"), name
        if sp["recompute"]:                                                          # a refresh before every epoch that ran but the first; the first finish's tables are returned
            assert o["recomputed_epochs"] == (o["epochs_run"] if "epochs_run" in o else sp["epochs"]) - 1
            assert not np.array_equal(o["refreshed_returns"], o["returns"], equal_nan=True) and np.array_equal(np.isnan(o["refreshed_returns"]), np.isnan(o["returns"]))
            rb, ok = o["refresh_bounds"], ~np.isnan(o["returns"])                  # the derived bounds: finite, positive (0 only for a one-step segment's normalised advantage)
            assert (rb["b_raw"][ok] > 0).all() and (rb["b_ret"][ok] > 0).all() and (rb["b_adv"][ok] >= 0).all() and all(np.isfinite(v[ok]).all() for v in rb.values())
        if sp["demo"] is not None:
            steps = len(o["losses"])
            assert len(o["demo_losses"]) == len(o["demo_rows"]) == steps and all(len(r) == 3 and len(set(r.tolist())) == 3 and max(r) < 7 for r in o["demo_rows"])
    if name in ("H", "M"):
        assert {k: v for k, v in sp.items() if k not in ("recompute", "vtrace", "latents", "seed", "precision")} == \
               {k: v for k, v in rc.spec("A").items() if k not in ("recompute", "vtrace", "latents", "seed", "precision")}
        assert sp["recompute"] and sp["vtrace"] == rc.H_BARS and [o["samples"] for o in outs] == [13, 12, 13]
        assert outs[2]["return_rms"] == outs[1]["return_rms"] and outs[1]["kl_coef"] == outs[0]["kl_coef_next"] != outs[0]["kl_coef"]
    if name == "H-gae":
        assert sp == dict(rc.spec("H"), vtrace=None)
    if name in ("I", "I-batch"):
        assert sp["vtrace"][0] != sp["vtrace"][1] and sp["k"] == 4 and sp["ddof"] == 1 and outs[0]["samples"] == 100
        assert cols[0]["truncs"].sum() == 2 and np.isfinite(outs[0]["refreshed_final_values"]).sum() == 2 and np.array_equal(np.isnan(outs[0]["refreshed_final_values"]), ~cols[0]["truncs"])
        assert rc.spec("I-batch") == dict(rc.spec("I"), normalize="batch")
    if name in ("J", "J-mse", "J-plain"):
        assert sp["k"] == 1 and "latent_stack" not in sp["on"] and sp["obs_given"] and (sp["demo"]["n"], sp["demo"]["batch"], sp["demo"]["decay"]) == (7, 3, 0.5)
        assert sp["demo"]["loss"] == ("mse" if name == "J-mse" else "nll") and len(sp["cycles"]) == (1 if name == "J-mse" else 2)
        given = rc.given_observation_state(sp)                                       # frozen: the statistics are the given ones behind every cycle
        assert all(o["observation_rms"]["count"] == given[0] and np.array_equal(o["observation_rms"]["mean"], given[1]) for o in outs)
        assert bool(sp["recompute"]) == (name != "J-plain") and (sp["vtrace"] is not None) == (name != "J-plain")
        np.random.seed(5)                                                            # the legacy stream is consumed as with the setting off: the shuffles alone
        for _ in range(sp["epochs"]):
            np.random.shuffle(np.arange(outs[0]["samples"]))
        want = np.random.get_state()[1].copy()
        np.random.seed(5)
        rc.Trainer(sp).update(cols[0])
        assert np.array_equal(np.random.get_state()[1], want)
    if name == "L":
        _, k3_1, k3_2 = rc.case_f_k3("L", cols[0])
        assert max(k3_1, k3_2) >= 2.0 * min(k3_1, k3_2), (k3_1, k3_2)
        assert outs[0]["epochs_run"] == 2 and outs[0]["stopped_early"] and outs[0]["recomputed_epochs"] == 1
        np.random.seed(5)
        for _ in range(2):
            np.random.shuffle(np.arange(outs[0]["samples"]))
        want = np.random.get_state()[1].copy()
        np.random.seed(5)
        rc.Trainer(sp).update(cols[0], target_kl=rc.case_target_kl("L", cols[0]))
        assert np.array_equal(np.random.get_state()[1], want)                          # the stream is left where two epochs leave it
    if name in rc.H_CASES:
        assert sp["on"] == tuple(o for o in rc.OPTIONAL if o != name[2:]) and sp["recompute"] and sp["vtrace"] == rc.H_BARS and len(sp["cycles"]) == 3
    if name in ("A", "D"):
        assert [o["samples"] for o in outs] == [13, 12, 13] and outs[0]["lengths"].tolist() == [5, 3, 5]       # ragged rows, minibatches 4, 4, 4 and a tail of 1 or none
        assert outs[1]["kl_coef"] == outs[0]["kl_coef_next"] != outs[0]["kl_coef"]                           # the chain is visible: beta moved
        assert outs[2]["return_rms"] == outs[1]["return_rms"] and outs[2]["observation_rms"]["count"] == outs[1]["observation_rms"]["count"]      # frozen
        assert outs[1]["return_rms"]["count"] == 25 and outs[1]["observation_rms"]["count"] == 25
    if name == "D":                                                                 # bf16x3: what the gradient tolerance adds to the parameter bound is stated
        assert rc.spec("D") == dict(rc.spec("A"), precision="bf16x3") and all(t > 0 for o in outs for t in o["param_tols"].values())
    if name == "K":                                                                 # the KL case: two steps, one clipped and one not, the floor <= 10 % of kl_bound
        assert len(outs[0]["losses"]) == 2 and max(fig["kl_floor_share"] + fig["kl_floor_share_steps"]) <= 0.1 and min(fig["kl_end"]) >= 0.19
    if name in ("B", "C"):
        segs = outs[0]["segment_list"]
        assert outs[0]["samples"] == 100 and len(segs) == 8 and cols[0]["truncs"][2, -1] and cols[0]["dones"][4, -1] and np.isfinite(cols[0]["final_values"]).sum() == 2
    if name == "F":
        _, k3_1, k3_2 = rc.case_f_k3("F", cols[0])
        assert max(k3_1, k3_2) >= 2.0 * min(k3_1, k3_2), (k3_1, k3_2)
        assert outs[0]["epochs_run"] == 2 and outs[0]["stopped_early"] and len(outs[0]["minibatch_adv_stats"]) == 2 * 4
        np.random.seed(5)
        for _ in range(2):
            np.random.shuffle(np.arange(outs[0]["samples"]))
        want = np.random.get_state()[1].copy()
        np.random.seed(5)
        rc.Trainer(sp).update(cols[0], target_kl=rc.case_target_kl("F", cols[0]))
        assert np.array_equal(np.random.get_state()[1], want)                          # the stream is left where two epochs leave it
    if name in rc.E_CASES:                                                           # the left-out setting's keys are absent
        absent = dict(grad_clip=("grad_norms", "clip_scales"), value_clip=(), reward_scaling=("return_rms", "scaled_rewards", "reward_scale_den"),
                      minibatch_norm=("minibatch_adv_stats", "minibatch_advantages"), observation_norm=("observation_rms", "observation_clip_fraction"),
                      kl_penalty=("kl", "kl_coef", "kl_coef_next"), latent_stack=())[name[2:]]
        assert all(k not in outs[0] for k in absent) and ("epochs" in outs[0]) == sp["diagnostics"]
        if name == "E-value_clip" and sp["diagnostics"]:
            assert "value_clip_fraction" not in outs[0]["epochs"][0]
        if name == "E-kl_penalty":
            assert "kl" not in outs[0]["losses"][0]
        if name == "E-latent_stack":
            assert outs[0]["raw_states"].shape[-1] == rc.Z + rc.N_MEAS


def test_both_buffer_classes_and_both_diagnostic_modes_run():
    assert {rc.spec(n)["kind"] for n in CASES} == {"rollout", "continuous"}
    assert {rc.spec(n)["diagnostics"] for n in rc.E_CASES} == {True, False}
    assert {rc.spec(n)["normalize"] for n in ("B", "C")} == {"segment", "batch"}


@pytest.mark.parametrize("name", CASES)
def test_the_fp32_twin_stays_inside_the_bounds(name):
    outs, twin, _ = runs(name)
    for cycle, (g, r) in enumerate(zip(twin, outs)):
        ratio, row = rc.worst(rc.compare(name, g, r, cycle=cycle))
        print(name, cycle, "worst distance / bound %.3g at %s" % (ratio, row))
        assert ratio <= 1.0, (name, cycle, row)


@pytest.mark.parametrize("mutant", rc.MUTANTS)
def test_every_mutant_is_seen_at_ten_times_a_bound(mutant):
    name = rc.NEWER_MUTANTS.get(mutant, "B" if mutant == "truncation_keeps_history" else "A")
    outs, twin, cols = runs(name)
    got, _, _ = rc.run_host(name, mutant=mutant, feed=cols)
    ratios = [rc.worst(rc.compare(name, g, r, twin=t, cycle=cycle)) for cycle, (g, r, t) in enumerate(zip(got, outs, twin))]
    print(mutant, ratios)
    assert max(r[0] for r in ratios) >= 10.0, (mutant, ratios)


def test_the_reference_stands_apart():
    src = open(rc.__file__.replace(".pyc", ".py")).read()
    names = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert names == {"collections", "numpy", "torch", "kl_penalty_cases", "latent_stack_cases", "oracle", "vtrace_cases", "demo_term_cases",
                     "advantage_recomputation_cases"}, names
    helpers = ("kl_penalty_cases.py", "latent_stack_cases.py", "vtrace_cases.py", "demo_term_cases.py", "advantage_recomputation_cases.py")
    for helper in helpers:                                                           # and so do the case modules it imports, for what it takes from them
        tree = ast.parse(open(os.path.join(os.path.dirname(rc.__file__), helper)).read())
        full = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names} | {n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
        # (advantage_recomputation_cases.parameters() takes the numpy-only initialiser mi355.init, as ppo_shape_cases does; the trainer calls neither)
        top = {m.split(".")[0] for m in full if not (helper == "advantage_recomputation_cases.py" and m == "mi355.init")}
        assert not top & {"rollout", "ppo", "mi355"}, (helper, top)
    init = ast.parse(open(os.path.join(os.path.dirname(os.path.dirname(rc.__file__)), "carla-ppo_amd", "mi355", "init.py")).read())
    assert {a.name.split(".")[0] for n in ast.walk(init) if isinstance(n, ast.Import) for a in n.names} | \
           {(n.module or "").split(".")[0] for n in ast.walk(init) if isinstance(n, ast.ImportFrom)} <= {"collections", "numpy", "sys", "zlib"}
