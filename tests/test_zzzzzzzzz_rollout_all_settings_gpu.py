"""Whole collect -> update cycles of both rollout buffers with EVERY setting on -- gradient clipping, value clipping, reward scaling, per-minibatch advantage
normalisation, observation normalisation, the adaptive KL penalty, latent stacking, the diagnostics pass with the KL stop, truncation, both normalisations --
against the float64 trainer of tests/rollout_trainer_cases.py (which calls nothing of rollout.py, ppo.py or mi355/ and carries its own parameters, Adam state, KL
coefficient, moments, carries and latent history from cycle to cycle).

Per case and cycle: collect on the device with injected noise and the scripted rewards / dones / truncations, read the tables back, run the update under a fixed numpy
seed, run the reference in float64 and float32 on the tables, and hold every number the update returns, the tables and the parameters to
rollout_trainer_cases.compare()'s bounds -- the project's own (see its docstring); tests/test_rollout_trainer_cases_host.py shows on the CPU that the fp32 twin
meets them and that each mis-ordering of the update is seen by them at 10 x or more.  Cases: rollout_trainer_cases.spec().  Case D is case A at
precision="bf16x3", held to that mode's README bounds with the fp32 mode's own distances (this module's run of case A) where a bound is stated relative to it; case
K is the one whose KL leaves the floor of kl_bound behind."""
import copy
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "carla-ppo_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rollout_trainer_cases as rc  # noqa: E402
from oracle import ppo_oracle as po  # noqa: E402
from oracle import vae_oracle as vo  # noqa: E402
from rollout_gpu_common import SENTINEL, bitwise, flat_state, make_vae, vae_params  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 5
PAD = 8


class World:
    def __init__(self, tmp):
        self.tmp, self._vaes, self.count, self.rows, self.last = tmp, {}, 0, {}, {}
        self.full = {}                                                               # per case and cycle, compare()'s rows as they are: (quantity, distance, bound)

    def vae(self, encoder):
        if encoder not in self._vaes:
            if encoder == "mlp":
                from vae.models import MlpVAE
                rng = np.random.RandomState(21)
                p = vo.init_mlp_vae_params(3, z_dim=rc.Z, source_shape=rc.MLP_SRC, target_shape=rc.MLP_SRC, encoder_sizes=rc.MLP_ENC, decoder_sizes=(8,))
                for k in p:
                    if k.endswith("bias"):
                        p[k] = (0.05 * rng.standard_normal(p[k].shape)).astype(np.float32)
                v = MlpVAE(np.array(rc.MLP_SRC), encoder_sizes=rc.MLP_ENC, decoder_sizes=(8,), z_dim=rc.Z, model_dir=str(self.tmp / "mlp_vae"), precision="fp32", training=False)
                v.set_weights(p)
                v.init_session(init_logging=False)
            else:
                v = make_vae(self.tmp / "conv_vae", vae_params())
            self._vaes[encoder] = v
        return self._vaes[encoder]

    def policy(self, sp):
        from ppo import PPO
        low, high = rc.bounds(sp["A"])
        self.count += 1
        m = PPO(np.array([rc.din_of(sp)]), po.ActionSpace(low, high), model_dir=str(self.tmp / ("ppo_%d" % self.count)), seed=2, precision=sp["precision"],
                **dict(rc.HP, learning_rate=sp["lr"]))
        m.set_weights(rc.initial_params(sp))
        if rc.din_of(sp) > 96:
            m.set_wide_inputs()
        m.init_session(init_logging=False)
        assert m.dev.fused_ok()
        return m


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return World(tmp_path_factory.mktemp("all_settings"))


def make_buffer(world, sp):
    from rollout import ContinuousRolloutBuffer, RolloutBuffer
    m = world.policy(sp)
    on = sp["on"]
    if "grad_clip" in on:
        m.set_max_grad_norm(sp["max_grad_norm"])
    if "value_clip" in on:
        m.set_value_clip(rc.VALUE_CLIP)
    if "kl_penalty" in on:
        m.set_kl_penalty(rc.KL_COEF, target=rc.KL_TARGET)
    cls = ContinuousRolloutBuffer if sp["kind"] == "continuous" else RolloutBuffer
    buf = cls.stacked(world.vae(sp["encoder"]), m, sp["E"], sp["T"], sp["k"], seed=3)
    if sp["obs_given"]:                                                              # given statistics, frozen in every cycle (settings() keeps them)
        count, mean, m2 = rc.given_observation_state(sp)
        buf.load_observation_normalization_state(dict(count=float(count), mean=mean, m2=m2, z_dim=rc.z_dim_of(sp), clip=rc.OBS_CLIP, epsilon=rc.STAT_EPS, frozen=True,
                                                      normalize_latents=True))
    settings(buf, sp, False)
    if sp["recompute"]:
        buf.set_advantage_recomputation(True)
    if sp["vtrace"] is not None:
        buf.set_vtrace(*sp["vtrace"])
    if sp["demo"] is not None:                                                       # the demonstration buffer: the same statistics, the scripted rows
        from rollout import DemonstrationBuffer
        dm, ds = sp["demo"], rc.demo_script(sp)
        db = DemonstrationBuffer(world.vae(sp["encoder"]), m, 16, chunk=4, seed=3)
        db.set_observation_normalization(buf.observation_normalization_state())
        db.add(ds["frames"], ds["meas"].astype(np.float64), ds["actions"])
        buf.set_demonstrations(db, dm["coef"], loss=dm["loss"], batch_size=dm["batch"], decay=dm["decay"], seed=dm["seed"])
    return buf, m


def settings(buf, sp, frozen):
    """The buffer's own settings (between two collections)."""
    on = sp["on"]
    if "reward_scaling" in on:
        buf.set_reward_scaling(clip=rc.REWARD_CLIP, epsilon=rc.STAT_EPS, frozen=frozen)
    if "minibatch_norm" in on:
        buf.set_minibatch_normalization(ddof=sp["ddof"])
    if "observation_norm" in on:
        buf.set_observation_normalization(clip=rc.OBS_CLIP, epsilon=rc.STAT_EPS, frozen=frozen or sp["obs_given"])


def collect(buf, sp, sc):
    """One scripted collection -> `col`, what rollout_trainer_cases.Trainer.update takes, read back from the tables and the calls' returns."""
    E, T, A, z = sp["E"], sp["T"], sp["A"], rc.z_dim_of(sp)
    shape = rc.MLP_SRC if sp["encoder"] == "mlp" else (80, 160, 3)
    rng = np.random.RandomState(sc["frame_seed"])
    frames = rng.randint(0, 256, (E, T + 1) + shape, dtype=np.uint8)
    final_frames = {(int(e), int(t)): rng.randint(0, 256, shape, dtype=np.uint8) for e, t in zip(*np.nonzero(sc["truncs"]))}
    meas = sc["meas"].astype(np.float64)
    latents = np.full((E, T + 1, z), np.nan, np.float32)
    buf.reset()

    def keep(lanes, slots, states):
        st32 = states.astype(np.float32)
        assert np.array_equal(st32.astype(np.float64), states)                        # the returned float64 state is the exact widening of fp32 values
        latents[lanes, slots] = st32[:, :z]
    if sp["kind"] == "rollout":
        live, t = np.arange(E), 0
        while len(live):
            _, _, states = buf.step(frames[live, t], meas[live, t], env_ids=live, noise=sc["noise"][live, t])
            keep(live, t, states)
            buf.outcome(sc["rewards"][live, t], sc["dones"][live, t], env_ids=live)
            t += 1
            live = live[~sc["dones"][live, t - 1] & (buf.lengths[live] < T)]
        need = buf.rows.stepped()
    else:
        lanes = np.arange(E)
        for t in range(T):
            _, _, states = buf.step(frames[:, t], meas[:, t], noise=sc["noise"][:, t])
            keep(lanes, t, states)
            buf.outcome(sc["rewards"][:, t], sc["dones"][:, t])
            cut = np.nonzero(sc["truncs"][:, t])[0]
            if len(cut):
                buf.truncate(np.stack([final_frames[(int(e), t)] for e in cut]), sc["final_meas"][cut, t].astype(np.float64), env_ids=cut)
        need = buf.rows.needs_bootstrap()
    lengths = buf.lengths.copy()
    assert np.array_equal(lengths, rc.lengths_of(sp, sc))
    if len(need):
        _, _, states = buf.bootstrap(frames[need, lengths[need]], meas[need, lengths[need]], env_ids=need)
        keep(need, lengths[need], states)
    fv = np.full((E, T), np.nan, np.float32)
    if sp["kind"] == "continuous":
        fv[sc["truncs"]] = buf.final_values.view(E, T + 1)[:, :T].cpu().numpy()[sc["truncs"]]
    col = dict(latents=latents, meas=sc["meas"], actions=buf.actions.view(E, T + 1, A).cpu().numpy(), values=buf.values.view(E, T + 1).cpu().numpy(), final_values=fv,
               rewards=sc["rewards"], dones=sc["dones"], truncs=sc["truncs"], lengths=lengths, noise=sc["noise"])
    if getattr(buf, "final_states", None) is not None:                               # advantage recomputation: the truncated steps' final observations as state rows
        fs = np.full((E, T, rc.din_of(sp)), np.nan, np.float32)
        fs[sc["truncs"]] = buf.final_states.view(E, T + 1, -1)[:, :T].cpu().numpy()[sc["truncs"]]
        col["final_states"] = fs
    if getattr(buf, "_demo", None) is not None:                                      # the demonstration term: the demonstration buffer's tables behind add()
        db = buf._demo["buffer"]
        col["demo_states"], col["demo_actions"] = db.states[:db.size].cpu().numpy(), db.expert_actions[:db.size].cpu().numpy()
    return col


def check_collection(name, cycle, buf, sp, col, tr, twin=None):
    """What the step recorded against the reference's forward of ITS parameters on ITS normalised states: values rel 1e-4 / abs 1e-5, actions rtol 1e-4 / atol 1e-5
    (in a later cycle this is what shows that the step read the updated policy and the merged statistics)."""
    E, T, A = sp["E"], sp["T"], sp["A"]
    _, states = tr.peek(col)
    rec = np.arange(T)[None, :] < col["lengths"][:, None]
    a_ref, v_ref = tr.predict(states[:, :T][rec], col["noise"][rec])
    a_dev, v_dev = col["actions"][:, :T][rec], col["values"][:, :T][rec]
    if twin is not None:                # the fp32 twin's forward of ITS parameters: tells a rounding effect of the trajectory from an error of the step
        a_tw, v_tw = twin.predict(twin.peek(col)[1][:, :T][rec], col["noise"][rec])
        print("%s cycle %d collection against the fp32 twin: actions max abs %.3e, values max abs %.3e" % (name, cycle, np.abs(a_dev - a_tw).max(), np.abs(v_dev - v_tw).max()))
    print("%s cycle %d collection: actions max abs %.3e, values max abs %.3e" % (name, cycle, np.abs(a_dev - a_ref).max(), np.abs(v_dev - v_ref).max()))
    assert np.allclose(a_dev, a_ref, rtol=1e-4, atol=1e-5), (name, cycle, "recorded actions", float(np.abs(a_dev - a_ref).max()))
    assert np.allclose(v_dev, v_ref, rtol=1e-4, atol=1e-5), (name, cycle, "recorded values", float(np.abs(v_dev - v_ref).max()))


def device_result(buf, m, sp, out):
    E, T = sp["E"], sp["T"]
    got = dict(out)
    raw = buf.raw_states if buf.raw_states is not None else buf.states
    got["raw_states"] = raw.view(E, T + 1, -1).cpu().numpy()
    got["states"] = buf.states.view(E, T + 1, -1).cpu().numpy()
    got["params"] = OrderedDict((k, np.asarray(v, np.float64)) for k, v in m.dev.export_params().items())
    return got


def check_finish(name, cycle, sp, col, out, tr):
    """The finish call on the rewards IT read: raw advantages and returns bitwise compute_gae per row / segment, the segment-normalised advantages bitwise the
    reference's (its sums in the kernels' order: rollout_trainer_cases.wave_sum), the batch-normalised ones within 1e-12 of the largest (tests/test_n_rollout_segments_gpu.py's
    bound for those sums); NaN beyond a row."""
    read = out["scaled_rewards"] if "reward_scaling" in sp["on"] else np.where(np.isnan(out["raw_advantages"]), np.nan, col["rewards"])
    raw, ret, adv = tr.finish(col, read)
    assert np.array_equal(out["raw_advantages"], raw, equal_nan=True) and np.array_equal(out["returns"], ret, equal_nan=True), (name, cycle, "raw advantages / returns")
    print("%s cycle %d finish: raw advantages and returns bitwise, normalised advantages max abs %.3e" % (name, cycle, np.nanmax(np.abs(out["advantages"] - adv))))
    if sp["kind"] == "continuous" and sp["normalize"] == "batch":
        assert np.array_equal(np.isnan(out["advantages"]), np.isnan(adv)) and np.nanmax(np.abs(out["advantages"] - adv)) <= 1e-12 * np.nanmax(np.abs(adv)), (name, cycle, "advantages")
    else:
        assert np.array_equal(out["advantages"], adv, equal_nan=True), (name, cycle, "advantages")


def moments(buf, sp):
    out = []
    if "reward_scaling" in sp["on"]:
        out.append(buf._reward_scaling["state"][:3].clone())
    if "observation_norm" in sp["on"]:
        out += [buf._obs_norm["state"].clone(), buf._obs_norm["mean32"].clone(), buf._obs_norm["inv32"].clone()]
    return out


def run_case(world, name, fp32_mode=None):
    """fp32_mode (a bf16x3 case): per cycle, {quantity: the fp32 mode's distance from its float64 reference} (world.rows of the same case in fp32 mode)."""
    import torch
    sp = rc.spec(name)
    buf, m = make_buffer(world, sp)
    tr64, tr32 = rc.Trainer(sp), rc.Trainer(sp, torch.float32)
    figures, world.rows[name], world.last[name] = [], [], []
    world.full[name] = []
    for cycle, frozen in enumerate(sp["cycles"]):
        buf.reset()                                                                  # (the settings change between two collections only)
        settings(buf, sp, frozen)
        col = collect(buf, sp, rc.script(sp, cycle))
        check_collection(name, cycle, buf, sp, col, tr64, tr32)
        target = rc.case_target_kl(name, col) if sp["target_kl"] is not None else None
        before = moments(buf, sp)
        at_start = None
        if cycle > 0 and "grad_clip" in sp["on"]:       # the reference on the DEVICE's parameters: the first norm of a later cycle is then compared like the first cycle's
            at_start = copy.deepcopy(tr64)
            at_start.params = OrderedDict((k, np.asarray(v, np.float64).copy()) for k, v in m.dev.export_params().items())
        kw = dict(normalize=sp["normalize"]) if sp["kind"] == "continuous" else {}
        np.random.seed(SEED + cycle)
        if sp["diagnostics"]:
            out = buf.update_with_diagnostics(rc.GAMMA, rc.LAM, num_epochs=sp["epochs"], batch_size=sp["batch"], target_kl=target, **kw)
        else:
            out = buf.update(rc.GAMMA, rc.LAM, num_epochs=sp["epochs"], batch_size=sp["batch"], **kw)
        stream = np.random.get_state()[1].copy()
        np.random.seed(SEED + cycle)
        r64 = tr64.update(col, frozen=frozen, target_kl=target)
        assert np.array_equal(np.random.get_state()[1], stream), (name, cycle, "numpy stream")       # the legacy stream is left where the reference's epochs leave it
        np.random.seed(SEED + cycle)
        r32 = tr32.update(col, frozen=frozen, target_kl=target)
        check_finish(name, cycle, sp, col, out, tr64)
        if at_start is not None:
            np.random.seed(SEED + cycle)
            first = at_start.update(col, frozen=frozen, target_kl=target)
            n_dev, n_ref, s_dev, s_ref = float(out["grad_norms"][0]), first["grad_norms"][0], float(out["clip_scales"][0]), first["clip_scales"][0]
            n_tol, s_tol = rc.ULP2 * n_ref, rc.ULP2 * s_ref
            if sp["precision"] == "bf16x3":                                          # what 1e-3 of each gradient tensor's max moves the norm by (compare())
                n_tol = first["grad_norm_tols"][0]
                s_tol = s_ref * n_tol / n_ref
            print("%s cycle %d first norm on the device's parameters: %.3e of %.3e; clip factor %.3e of %.3e" % (name, cycle, abs(n_dev - n_ref), n_tol, abs(s_dev - s_ref), s_tol))
            assert abs(n_dev - n_ref) <= n_tol and abs(s_dev - s_ref) <= s_tol, (name, cycle, "first norm", n_dev, n_ref, s_dev, s_ref)
        print("%s cycle %d margins: ratio %.3e, value %.3e" % (name, cycle, r64["margins"]["ratio"].min(), r64["margins"]["value"].min() if len(r64["margins"]["value"]) else np.nan))
        got = device_result(buf, m, sp, out)
        rows = rc.compare(name, got, r64, twin=r32, cycle=cycle, fp32_mode=None if fp32_mode is None else fp32_mode[cycle])
        world.rows[name].append({q: err for q, err, _ in rows})
        world.full.setdefault(name, []).append(rows)
        world.last[name].append((got, r64))
        ratio, row = rc.worst(rows)
        tw_ratio, tw_row = rc.worst(rc.compare(name, r32, r64, cycle=cycle))
        print("%s cycle %d: worst distance / bound %.3g at %s; the fp32 twin's %.3g at %s" % (name, cycle, ratio, row, tw_ratio, tw_row))
        traj = rc.trajectory_errors(got["params"], r32["params"], r64["params"], r64["p0"])
        for k, e_d, e_t, scale in traj:
            print("    %-34s device %.3e  twin %.3e  (RMS update error / max |update|)" % (k, e_d / scale, e_t / scale))
        if sp["precision"] == "bf16x3":                                               # the rule of tests/test_j_ppo_bf16x3_gpu.py alone, as a figure: 2 x the fp32 mode + 2e-4
            for k, e_d, _, scale in traj:
                print("    %-34s bf16x3 %.3e, fp32 mode %.3e; the gradient tolerance alone would allow %.3e (of max |update|)"
                      % (k, e_d / scale, fp32_mode[cycle].get("params " + k, 0.0) / scale, r64["param_tols"][k] / scale))
        for q, err, bound in rows:
            if q.split("[")[0] in ("loss", "value_loss", "kl", "grad_norm", "approx_kl", "explained_variance", "kl.kl") and bound > 0 and err / bound > 0.05:
                print("    %-24s %.3e of %.3e" % (q, err, bound))
        bad = [(q, err, bound) for q, err, bound in rows if not err <= bound]
        assert not bad, (name, cycle, bad)
        if "minibatch_norm" in sp["on"]:                                             # the fp32 table of the last epoch: (float) of the same quotient, one ulp for the 1e-9 of its inputs
            g, r = out["minibatch_advantages"], r64["minibatch_advantages"]
            tol = r64["minibatch_advantages_tol"][~np.isnan(r)] if "minibatch_advantages_tol" in r64 else 0.0      # behind a refresh: what its raw advantages' bounds allow
            assert np.array_equal(np.isnan(g), np.isnan(r)) and (np.abs(g - r)[~np.isnan(r)] <= np.spacing(np.abs(r[~np.isnan(r)])) + tol).all(), (name, cycle)
        if frozen:
            assert bitwise(moments(buf, sp), before), (name, cycle)
        elif before:
            assert not bitwise(moments(buf, sp), before), (name, cycle)
        if "kl_penalty" in sp["on"]:
            assert m.kl_penalty == r64["kl_coef_next"], (name, cycle)
        figures.append((out, r64))
        m.episode_counter += 1                                                       # the next cycle runs at float32(lr) x float32(decay) ^ episode
        tr64.episode += 1
        tr32.episode += 1
    print("%s conditions on the tables the device collected: %s" % (name, rc.check_conditions(name, [r for _, r in figures])))      # the margins the exact counts rest on
    return figures


def test_a_high_kl_case_leaves_the_floor_of_kl_bound_behind(world):
    """Case K: one epoch of two steps at learning rate 2e-2.  The second step's KL and the end-of-cycle KL are large enough for the floor of kl_bound to be at most
    10 % of the bound (check_conditions asserts it on the tables collected here), so the 1e-4 relative part is what holds `kl` and `kl_penalty`."""
    (out, ref), = run_case(world, "K")
    shares = [l["kl_floor_share"] for l in ref["losses"][1:]] + [ref["kl_floor_share"]]
    print("K: floor share of kl_bound %s, per-step KL %s, end-of-cycle KL %.4f" % (np.round(shares, 4), [round(l["kl"], 4) for l in out["losses"]], out["kl"]["kl"]))
    assert max(shares) <= rc.KL_FLOOR_SHARE and len(out["losses"]) == 2


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_chained_cycles_with_every_setting_on(world, name):
    figures = run_case(world, name)
    if name == "A":                                                                  # the chain, seen from the device: beta, the moments, the Adam step count
        (o1, _), (o2, _), (o3, _) = figures
        assert o2["kl_coef"] == o1["kl_coef_next"] != o1["kl_coef"] and o3["kl_coef"] == o2["kl_coef_next"]
        assert o2["return_rms"]["count"] == 25 and o3["return_rms"] == o2["return_rms"] and o3["observation_rms"]["count"] == 25
        assert o1["reward_clip_fraction"] > 0 and o1["observation_clip_fraction"].max() > 0


def test_case_a_in_bf16x3(world):
    """Case D.  The fp32 mode's distances are case A's (run here if that test has not run)."""
    if "A" not in world.rows:
        run_case(world, "A")
    figures = run_case(world, "D", fp32_mode=world.rows["A"])
    assert len(figures) == 3


@pytest.mark.parametrize("name", rc.E_CASES)
def test_leave_one_out(world, name):
    (out, ref), = run_case(world, name)
    assert ("epochs" in out) == rc.spec(name)["diagnostics"]


def test_the_kl_stop_fires(world):
    (out, ref), = run_case(world, "F")
    assert out["epochs_run"] == 2 and out["stopped_early"] and len(out["epochs"]) == 2
    assert out["minibatch_adv_stats"].shape == (2 * 4, 3) and len(out["losses"]) == 2 * 4    # only the epochs that ran
    assert out["kl_coef_next"] == ref["kl_coef_next"]


def test_conv_encoder_wide_inputs(world):
    run_case(world, "G")


def padded(t, value=SENTINEL):
    import torch
    big = torch.full((t.numel() + PAD,), value, dtype=t.dtype, device=t.device)
    big[:t.numel()] = t.reshape(-1)
    return big[:t.numel()].view(t.shape), big[t.numel():]


def test_two_runs_are_bitwise_equal_and_write_nothing_behind_the_tables(world):
    """Case A's first update twice from the same tables and the same state: every number, the parameters and the Adam slots bitwise; 8 sentinels behind each table
    the update writes survive."""
    import torch
    sp = rc.spec("A")
    buf, m = make_buffer(world, sp)
    collect(buf, sp, rc.script(sp, 0))
    pads = []
    for attr in ("returns", "advantages", "logp_old"):
        t, pad = padded(getattr(buf, attr))
        setattr(buf, attr, t)
        pads.append(pad)
    buf.mean_old, pad = padded(torch.zeros(buf.n_table_rows, sp["A"], device=buf.device))
    pads.append(pad)
    buf._minibatch_advantages, pad = padded(torch.zeros(buf.n_table_rows, device=buf.device))
    pads.append(pad)
    live = [m.dev.params, m.dev.adam_m, m.dev.adam_v, m.dev.params_old, buf._reward_scaling["state"], buf._reward_scaling["carry"]]
    live += [buf._obs_norm[k] for k in ("state", "mean32", "inv32")]
    saved = [t.clone() for t in live]
    host = (m.beta1_power, m.beta2_power, m.kl_penalty, m.train_step_counter)

    def once():
        np.random.seed(SEED)
        out = buf.update_with_diagnostics(rc.GAMMA, rc.LAM, num_epochs=sp["epochs"], batch_size=sp["batch"])
        return out, [t.clone() for t in flat_state(m)] + moments(buf, sp)
    out1, state1 = once()
    for t, s in zip(live, saved):
        t.copy_(s)
    m.beta1_power, m.beta2_power, m.kl_penalty, m.train_step_counter = host
    out2, state2 = once()
    assert bitwise(state1, state2) and not bitwise(state1[0], saved[0])
    assert out1["losses"] == out2["losses"] and out1["epochs"] == out2["epochs"] and out1["kl"] == out2["kl"] and out1["kl_coef_next"] == out2["kl_coef_next"]
    for k in ("returns", "advantages", "raw_advantages", "grad_norms", "clip_scales", "minibatch_adv_stats", "minibatch_advantages", "scaled_rewards", "discounted_returns",
              "return_carry", "observation_clip_fraction"):
        assert np.array_equal(out1[k], out2[k], equal_nan=True), k
    assert out1["return_rms"] == out2["return_rms"] and all(np.array_equal(out1["observation_rms"][k], out2["observation_rms"][k]) for k in ("count", "mean", "var"))
    torch.cuda.synchronize()
    assert all(bool((p == SENTINEL).all()) for p in pads)
