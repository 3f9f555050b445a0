"""A float64 restatement of a WHOLE rollout-buffer update with every setting on, and the cases it is run at (test infrastructure; used by
test_rollout_trainer_cases_host.py, test_zzzzzzzzz_rollout_all_settings_gpu.py and test_zzzzzzzzzzzzzzz_rollout_newer_settings_gpu.py).

Trainer is a plain numpy / torch-CPU PPO trainer.  It imports nothing of rollout.py, ppo.py or mi355/ and knows none of their stages; the pieces it shares with the
other references are oracle.ppo_oracle (policy_forward, normal_log_prob, compute_gae, AdamTF), oracle.vae_oracle (the MlpVAE encoder of the scripted frames),
kl_penalty_cases (kl_terms, kl_bound, adapted), latent_stack_cases (stack_rows, shift: copying) and, for the newer settings, vtrace_cases, demo_term_cases and
advantage_recomputation_cases (below).  Everything else is written here from the definitions in include/mi355_carla.h.  It keeps its own state across
updates: parameters, Adam slots and powers, the episode counter behind the learning rate, the KL coefficient, the reward-scaling moments and per-lane carries, the
observation moments, the latent history and its fresh flags.

One cycle takes what a collection left behind AS DATA (`col`: the latents and measurements of every slot, the recorded actions and values, final_values, and the
host rewards / dones / truncs / lengths) and states, in order:
  assemble     s = [z_t | the k - 1 latents before it | measurements], a fresh lane repeating its own latent; a done or a truncation makes the lane fresh
  rewards      G = G gamma + r from the lane's carry (0 behind a done or a truncation); the collection's G merged into {count, mean, M2} (Chan) unless frozen;
               r / sqrt(M2 / count + epsilon) clamped into +-clip
  finish       compute_gae per row / per segment (a truncated segment bootstraps from final_values, a terminal one from 0), returns = A + V, advantages normalised
               per segment or over the batch ((a - mean) / (std + 1e-8), population std)
  states       clamp((s - mean) / sqrt(M2 / count + epsilon), +-clip) from the moments AS THEY ARE BEFORE this update's merge
  old policy   theta_old = theta; log pi_old and the old means of every valid row
  epochs       np.random.shuffle (the legacy stream) of the valid rows, minibatches of batch_size (the last one partial); per minibatch the advantage normalised
               from the RAW advantages (ddof 0 / 1; rounded to fp32, the table's type), the clipped surrogate, max((V - R)^2, (V_c - R)^2) around the recorded
               values, the entropy term, beta x mean KL(pi_old || pi_theta); autograd; the global norm over the 13 tensors and the clip factor; TF-Adam at
               float32(lr) x float32(decay) ^ episode
  diagnostics  per epoch over all valid rows: k3 / k1 KL, clip fraction, mean ratio, value error and explained variance on the returns the steps read (those of
               the scaled rewards), the three value-clip fractions; the KL stop with a plain `>`
  afterwards   the exact KL over all valid rows under the final parameters, the coefficient's adaptation, the observation moments' merge (behind the epochs) unless
               frozen

dtype float64 is the reference.  dtype float32 is the project's "fp32 oracle" twin: the forward, autograd and Adam in float32 and the observation normalised by the
fp32 pair (float32(mean), float32(1 / sqrt(var + epsilon)); one subtract, one multiply) -- what an honest fp32 implementation does; the stages the header defines in
fp64 (reward scaling, GAE, the normalisations, the moments, every diagnostic sum) stay fp64 in both.  The tables' types are data: returns, advantages and states are
rounded to fp32 where the update reads them from an fp32 table (the twin's states; the reference keeps its float64 states).

mutant= (never passed by the GPU test) wires ONE of the mis-orderings the suite could not see before this file (MUTANTS).  test_rollout_trainer_cases_host.py shows
that each moves an asserted quantity by at least 10 x its bound.

THE NEWER SETTINGS (cases H .. M; test_zzzzzzzzzzzzzzz_rollout_newer_settings_gpu.py), written from the header and the module docstring of rollout.py like the rest;
formulas that vtrace_cases (deltas, recurrence), demo_term_cases (demo_terms, demonstration_rows) and advantage_recomputation_cases (the value bound) already state
in float64 are taken from there:
  refresh      (recompute) before every epoch that runs but the first: the value net under the current parameters over every recorded row and every recorded
               bootstrap slot of the states the steps read (normalised, stacked), in the continuous buffer also over the truncated steps' final observations
               (col["final_states"], data), each rounded to fp32 (values_now / final_values_now); the finish again on those values with the rewards the first
               finish read (the scaled ones), the same segments and normalisation.  From then on the steps gather the refreshed returns and advantages, the minibatch
               normalisation reads the refreshed raw advantages and the diagnostics the refreshed returns; value clipping keeps the RECORDED values as V_old, and the
               result's returns / advantages / raw_advantages stay the first finish's.  A KL stop ends the refreshes with the epochs
  V-trace      (vtrace = (rho_bar, c_bar)) on that refresh: w = exp(log pi_theta - log pi_old) per recorded step from the two fp32 tables, log pi_old the update's ONE
               cache (which the steps keep reading); mi_rollout_finish_vtrace's recurrence; RolloutBuffer by mi_rollout_finish's successor rule, the continuous
               buffer by the segment entries'
  demo term    (demo) per step min(batch_size, n) rows by the documented rule from the setting's own RandomState(seed); loss = L_ppo(PPO rows) + float32(coef) x
               clone_loss(demonstration rows), one gradient (the global norm sees all of it), one Adam step; every other mean runs over the PPO rows; coef *= decay
               behind the update.  The demonstration rows' states and expert actions are data (col["demo_states"], col["demo_actions"])
THE REFRESHED TABLES' BOUNDS are derived per entry and have no constant of their own: values by advantage_recomputation_cases' rel 1e-4 / abs 1e-5; weights by
|dw| <= w expm1(1e-4 (absolute terms of log pi_theta) + 1e-4 (those of log pi_old)); raw advantages and returns by the finish's own recurrence run on those bounds
(Trainer.finish_bounds), the normalised advantages through normalised_bound(); the minibatch statistics and the minibatch table behind a refresh likewise.  Where such a
bound is looser than 100 x the fp32 twin's distance in every case (TWIN_HELD), the quantity is also held to 4 x the twin's distance.
latents="encoder" (the newer cases): the host test's collections hold the encoder oracle's latents of the very frames the GPU test feeds, so the conditions asserted
on the CPU are the device's up to the encoder's fp32 rounding.

THE STATE BOUND (observation normalisation, GPU test).  The device forms n32 = fl((fl(s - m32)) i32) with m32 = fl(mean_d), i32 = fl(1 / sqrt(var_d + eps)) from ITS
fp64 moments; the reference n = (s - mean) / sqrt(var + eps) in float64.  With u = 2^-24 (round to nearest): |fl(mean) - mean| <= u |mean|, so the subtraction is off by
at most u |mean| + u |s - m32|; the inverse by u i32; the product by u |n|.  The moments' own bounds (mean: 1e-12 max|x|, M2 / count: 1e-9 relative) add 1e-12 max|x| i
and 0.5e-9 |n|.  Together  |n32 - n| <= u (|mean| + |s - mean|) i + 2 u |n| + 1e-12 max|x| i + 1e-9 |n|  (state_bound()), which for a centred column is the 1 ulp of the
observation row (|n| 2^-23) plus the share of the mean's rounding: no tolerance of its own.  A clamped entry is +-clip exactly on both sides.

Cases (spec()): the encoder is the MlpVAE 72 -> (36,) -> 8 on (4, 6, 3) frames (G: the ConvVAE at 64 latents), 3 measurements.  The policy is the PPO class's own
500 / 300 trunks (the class has no other; 36 / 20 exists at the engine level only).  Learning rate 1e-3 with lr_decay 0.9, and the episode counter is advanced between
two cycles, so the cycles run at different learning rates; max_grad_norm 2.0 (at 0.5 every step of every case was clipped), eps_v 0.2, beta 0.5 towards a KL of
0.005 (so that beta doubles from cycle to cycle and a stale coefficient shows), both clamps at 2.5.  The script seeds are pinned so that the margins below hold on
the tables the device collects (profiles/r32_rollout_all_settings.md has the scans).

THE KL CASE (K).  Cases A .. G end their cycles at KLs of 0.006 .. 0.07 (asserted >= 1e-3), where the floor of kl_bound is 0.2 .. 0.75 of the bound.  Case K is
one epoch of two steps (13 samples in minibatches of 8 and 5) at learning rate 2e-2: Adam's first step moves every parameter by the learning rate, so the second
step's KL and the end-of-cycle KL are about 0.5 while the update is two steps long and the float32 trajectory has no time to leave the float64 one (the twin's worst
distance is 0.2 of its bound).  check_conditions() asserts for it that the floor is at most 10 % of kl_bound at every step behind the first (whose KL is exactly 0 in
every cycle) and at the end of the cycle, so there the 1e-4 relative part holds `kl` and `kl_penalty`.  Its max_grad_norm is 20, so that the first step (norm 6 .. 10)
is not clipped and the second (norm 40 .. 250) is.

THE bf16x3 CASE (D) is case A with precision="bf16x3", held to the bounds the README states for that mode ("Numerical tolerances", the PPO bf16x3 column); `fp32
mode` below is the device's own run of case A, each on the tables it collected itself:
  loss scalars, per-step KL   as in fp32 mode (1e-4; kl_bound)
  diagnostics, KL summary     1e-4 relative, else 4 x the fp32 mode's distance (the rule of tests/test_p_rollout_diagnostics_gpu.py); counts exact
  parameters                  no further from the float64 trajectory than 2 x the fp32 mode + 2e-4 of the update (the README's rule for a bf16x3 update,
                              tests/test_j_ppo_bf16x3_gpu.py's C3 test)
  norms, clip factors         against float64 the norm inherits the gradients' tolerance, 1e-3 of each tensor's max: | |g'| - |g| | <= |g' - g| <=
                              1e-3 sqrt(sum_k n_k max_k^2) (grad_norm_tols; n_k entries in tensor k), the factor c / norm the same relatively
  tables, counts, moments     as in fp32 mode (the step and the finish have one precision)
THE bf16x3 PARAMETER BOUND is the tighter of two that can be stated.  The other is what the gradient tolerance alone allows Adam to differ by
(propagate_gradient_tolerance(), reported as `param_tols`, NOT asserted): with every gradient entry off by at most a_t = 1e-3 max_k at step t, m is off by at most
A_m (m's recurrence run on a_t) and sqrt(v) by at most A_v (v's recurrence on a_t^2, Minkowski), so one step differs by at most
alpha (A_m + |m| / (sqrt(v) + eps) A_v) / (max(sqrt(v) - A_v, 0) + eps), and never by more than twice the largest step Adam can take (Cauchy-Schwarz over the two
recurrences).  Entries whose gradient is small against their tensor's max (dead units) reach that cap, so the RMS over a kernel is 0.6 .. 2.5 x the largest update: a
tolerance of 1e-3 of max on the gradients says next to nothing about parameters behind Adam, and any trajectory error up to that size "follows from" it.  The device
is at 1e-6 .. 2.6e-5 of the largest update, inside the tighter rule by 8 x and more (profile).
"""
from collections import OrderedDict

import numpy as np
import torch

import advantage_recomputation_cases as ar
import demo_term_cases as dc
import kl_penalty_cases as kc
import latent_stack_cases as lc
import vtrace_cases as vc
from oracle import ppo_oracle as po
from oracle import vae_oracle as vo

GAMMA, LAM = 0.99, 0.95
Z, N_MEAS = 8, 3
MLP_SRC, MLP_ENC = (4, 6, 3), (36,)
HP = dict(learning_rate=1e-3, lr_decay=0.9, epsilon=0.2, value_scale=1.0, entropy_scale=0.01, initial_std=1.0)
MAX_GRAD_NORM, VALUE_CLIP, KL_COEF, KL_TARGET = 2.0, 0.2, 0.5, 0.005
REWARD_CLIP, OBS_CLIP, STAT_EPS = 2.5, 2.5, 1e-8
K_LR, K_MAX_GRAD_NORM, K_SEED, KL_FLOOR_SHARE = 2e-2, 20.0, 42, 0.10
GRAD_TOL_X3 = 1e-3                                       # bf16x3: each gradient tensor within 1e-3 of its max (README, "gradients (each tensor, of its max)")
OPTIONAL = ("grad_clip", "value_clip", "reward_scaling", "minibatch_norm", "observation_norm", "kl_penalty", "latent_stack")
MUTANTS = ("finish_reads_unscaled_rewards", "returns_of_unscaled_rewards", "old_policy_on_raw_states", "minibatch_norm_of_normalised", "penalty_behind_clip",
           "observation_merge_before_epochs", "observation_merge_twice", "truncation_keeps_history", "kl_coef_next_unused")
# the newer settings (advantage recomputation, V-trace, the demonstration term): each mutant with the case test_rollout_trainer_cases_host.py shows it in
NEWER_MUTANTS = OrderedDict([
    ("value_clip_reads_refreshed_values", "H"), ("refresh_reads_unscaled_rewards", "H"), ("refresh_values_raw_states", "H"), ("refresh_recaches_logp_old", "H"),
    ("minibatch_norm_reads_first_raw_advantages", "H"), ("diagnostics_read_first_returns", "H"), ("result_returns_are_refreshed", "H"), ("vtrace_bars_swapped", "I"),
    ("refresh_bootstraps_from_recorded_final_values", "I"), ("refresh_before_epoch_1", "H"), ("no_refresh", "H"), ("stale_bootstrap_slots", "H"),
    ("refresh_behind_the_kl_stop", "L"), ("penalty_and_value_terms_over_demo_rows", "J"), ("demo_rows_from_the_legacy_stream", "J"), ("demo_coef_next_unused", "J")])
assert set(ar.MUTANTS) <= set(NEWER_MUTANTS)
MUTANTS = MUTANTS + tuple(NEWER_MUTANTS)
H_BARS, I_BARS = (1.0, 1.0), (1.03, 0.97)                # (rho_bar, c_bar) of V-trace: H the defaults, I two bars that differ
DEMO = dict(n=7, batch=3, coef=0.4, decay=0.5, loss="nll", seed=11)      # 7 rows in minibatches of 3: a fresh permutation every other step
GIVEN_OBS_ROWS = 32                                      # case J: the observation statistics it is given are the moments of this many scripted rows
H_SEED, I_SEED, J_SEED, L_SEED = 25, 31, 25, 14
H_OFF_SEEDS = dict(value_clip=28, observation_norm=26)   # leave-one-out cases whose margins H's own script misses (profiles/r41_rollout_newer_settings.md)
TWIN_HELD = ("refreshed_importance_weights", "refreshed_advantages")
LOGP_REL = 1e-4                                         # log pi: 1e-4 of the sum of its absolute terms (tests/test_zzzzzzzzzzzzzz_vtrace_gpu.py, behaviour_cloning_cases)

# the margins of the conditions (check_conditions)
RATIO_MARGIN, VALUE_MARGIN, CLAMP_MARGIN, NORM_MARGIN, KL_STOP_MARGIN, KL_MIN = 1e-4, 1e-4, 1e-6, 1e-3, 0.10, 1e-3
# the project's tolerances, by their README rows
LOSS_REL, DIAG_REL, TRAJ_FACTOR, TRAJ_FLOOR, ULP2 = 1e-4, 1e-4, 2.0, 2e-4, 2.4e-7
MOMENT_MEAN, MOMENT_VAR = 1e-12, 1e-9
# approx_kl_k1 = -mean(log pi - log pi_old): log pi_old is READ from an fp32 table and log pi is formed in fp32, so each carries half an ulp of its own magnitude
# before any arithmetic error: |d k1| <= 2 x 2^-24 max |log pi_old| whatever k1 itself is -- and k1 cancels to 1e-4 and less at a first epoch.  This floor is the
# number format's, added to the 1e-4 relative of that ONE statistic; k3, the mean ratio, the value error and the explained variance keep 1e-4 relative alone.
K1_FLOOR = 2.0 * 2.0 ** -24
# keys that only one side holds: the reference's working figures, and tables of the device's result that are compared as tables
NOT_RETURNED = ("params", "p0", "margins", "segment_list", "state_bound", "logp_old_max", "raw_states", "states", "kl_floor_share",
                "grad_norm_tols", "param_tols", "values", "bootstrap_values", "segments", "segment_truncated", "final_values", "refresh_bounds", "refresh_moved",
                "demo_states", "demo_actions", "minibatch_stat_tols", "minibatch_advantages_tol")
U32 = 2.0 ** -24


def spec(name):
    """-> the case's dict.  kind: "rollout" (RolloutBuffer) or "continuous"; on: the optional settings that are on; cycles: per cycle, is it frozen."""
    base = dict(kind="rollout", E=3, T=5, A=2, batch=4, epochs=3, k=2, ddof=0, normalize="segment", cycles=(False,), on=OPTIONAL, diagnostics=True, target_kl=None,
                precision="fp32", encoder="mlp", seed=25, lr=HP["learning_rate"], max_grad_norm=MAX_GRAD_NORM, kl_share_max=None,
                recompute=False, vtrace=None, demo=None, obs_given=False, latents="synthetic")
    # the newer settings (recompute: advantage recomputation; vtrace: None or (rho_bar, c_bar); demo: None or the demonstration term's settings; obs_given: the
    # observation statistics are given and frozen in every cycle; latents "encoder": the host test's collections hold the encoder oracle's latents of the frames the
    # GPU test feeds, so that the conditions it asserts are those of the device's tables up to the encoder's rounding)
    if name == "H":
        return dict(spec("A"), recompute=True, vtrace=H_BARS, latents="encoder", seed=H_SEED)
    if name == "H-gae":
        return dict(spec("H"), vtrace=None)
    if name == "I":
        return dict(spec("B"), recompute=True, vtrace=I_BARS, latents="encoder", seed=I_SEED)
    if name == "I-batch":
        return dict(spec("I"), normalize="batch")
    if name == "J":                                                                  # (the demonstration term refuses a stacked buffer: k = 1)
        return dict(spec("H"), k=1, on=tuple(o for o in OPTIONAL if o != "latent_stack"), obs_given=True, demo=dict(DEMO), cycles=(False, False), seed=J_SEED)
    if name == "J-mse":
        return dict(spec("J"), demo=dict(DEMO, loss="mse"), cycles=(False,))
    if name == "J-plain":
        return dict(spec("J"), recompute=False, vtrace=None)
    if name == "L":                                                                  # one cycle, as case F: the target is placed on the reference's own first update
        return dict(spec("H"), cycles=(False,), target_kl="geometric mean of the reference's epoch-1 and epoch-2 k3", seed=L_SEED)
    if name == "M":
        return dict(spec("H"), precision="bf16x3")
    if name.startswith("H-") and name[2:] in OPTIONAL:
        off = name[2:]
        return dict(spec("H"), on=tuple(o for o in OPTIONAL if o != off), diagnostics=OPTIONAL.index(off) % 2 == 0, k=1 if off == "latent_stack" else 2,
                    seed=H_OFF_SEEDS.get(off, H_SEED))
    if name == "A":
        return dict(base, cycles=(False, False, True))
    if name == "D":
        return dict(spec("A"), precision="bf16x3")
    if name == "K":                                                                  # one epoch of two steps at a high learning rate: see "THE KL CASE" above
        return dict(base, batch=8, epochs=1, lr=K_LR, max_grad_norm=K_MAX_GRAD_NORM, kl_share_max=KL_FLOOR_SHARE, seed=K_SEED)
    if name == "B":
        return dict(base, kind="continuous", E=5, T=20, A=3, batch=32, k=4, ddof=1, cycles=(False, False), seed=31)
    if name == "C":
        return dict(spec("B"), normalize="batch")
    if name.startswith("E-"):
        off = name[2:]
        assert off in OPTIONAL, name
        return dict(base, on=tuple(o for o in OPTIONAL if o != off), diagnostics=OPTIONAL.index(off) % 2 == 0, k=1 if off == "latent_stack" else 2, seed=13)
    if name == "F":
        return dict(base, target_kl="geometric mean of the reference's epoch-1 and epoch-2 k3", seed=14)
    if name == "G":
        return dict(base, encoder="conv", seed=17)
    raise KeyError(name)


E_CASES = tuple("E-" + o for o in OPTIONAL)
H_CASES = tuple("H-" + o for o in OPTIONAL)              # leave-one-out over the OLDER settings on top of H
NEWER_CASES = ("H", "H-gae", "I", "I-batch", "J", "J-mse", "J-plain", "L", "M") + H_CASES


def z_dim_of(sp):
    return 64 if sp["encoder"] == "conv" else Z


def din_of(sp):
    return sp["k"] * z_dim_of(sp) + N_MEAS


def bounds(A):
    """The action bounds: the reference's for 2 actions, ppo_shape_cases' rule otherwise (no two actions alike)."""
    if A == 2:
        return np.array([-1.0, 0.0], np.float32), np.array([1.0, 1.0], np.float32)
    a = np.arange(A)
    return (-1.0 - 0.25 * a).astype(np.float32), (0.5 + 0.5 * (a % 3)).astype(np.float32)


def initial_params(sp):
    p = po.init_ppo_params(2, din_of(sp), sp["A"], HP["initial_std"])
    rng = np.random.RandomState(40 + sp["A"])
    for k in p:
        if k.endswith("bias"):
            p[k] = (0.05 * rng.standard_normal(p[k].shape)).astype(np.float32)
    return p


# ------------------------------------------------------------------------------------------------------------------------------------ the script of a collection
def script(sp, cycle):
    """What the simulator does in one collection, as arrays: measurements [E, T + 1, 3] (slot lengths[e] is the bootstrap observation), noise [E, T, A], rewards,
    dones, truncs [E, T], the measurements of a truncated episode's final observation [E, T, 3], and the seeds of the frames.  One large reward and one large
    measurement are planted per cycle so that both clamps fire."""
    E, T, A = sp["E"], sp["T"], sp["A"]
    rng = np.random.RandomState(1000 * sp["seed"] + cycle)
    meas = np.stack([rng.uniform(-1, 1, (E, T + 1)), rng.uniform(0, 1, (E, T + 1)), rng.uniform(0, 2, (E, T + 1))], axis=2)
    final_meas = np.stack([rng.uniform(-1, 1, (E, T)), rng.uniform(0, 1, (E, T)), rng.uniform(0, 2, (E, T))], axis=2)
    noise = rng.standard_normal((E, T, A)).astype(np.float32)
    rewards = rng.uniform(0, 1, (E, T))
    dones, truncs = np.zeros((E, T), bool), np.zeros((E, T), bool)
    if sp["kind"] == "rollout":
        dones[1, 2 - cycle % 2] = True                                               # ragged rows with one terminal: lane 1 ends at its step 3 (2 in odd cycles)
        if "reward_scaling" in sp["on"]:                                             # (each planted where its clamp exists: without the setting it would only ill-condition the sums)
            rewards[2, T - 1] = 40.0                                                 # the planted reward: a row's last step, so that its G does not run on
        if "observation_norm" in sp["on"]:
            meas[0, 1, 2] = 60.0                                                     # the planted measurement
    else:
        dones[1, 6], dones[3, 11], dones[4, T - 1] = True, True, True                # dones in mid-lane, a lane ending in a done
        truncs[0, 8], truncs[2, T - 1] = True, True                                  # two truncations, one at a lane's last slot
        rewards[1, 6] = 100.0                                                        # in front of a done
        meas[3, 4, 2] = 300.0
    return dict(meas=meas.astype(np.float32), final_meas=final_meas.astype(np.float32), noise=noise, rewards=rewards, dones=dones, truncs=truncs,
                frame_seed=5000 * sp["seed"] + cycle)


def lengths_of(sp, sc):
    """Recorded steps per lane: a RolloutBuffer row ends at its done or at the horizon; a continuous lane is always full."""
    E, T = sp["E"], sp["T"]
    if sp["kind"] == "continuous":
        return np.full(E, T, np.int32)
    first = np.where(sc["dones"].any(1), sc["dones"].argmax(1) + 1, T)
    return first.astype(np.int32)


def synthetic_latents(sp, cycle):
    """Host test: latents in place of an encoder.  -> (latents [E, T + 1, z], final latents [E, T, z]), float32."""
    rng = np.random.RandomState(7000 * sp["seed"] + cycle)
    z = z_dim_of(sp)
    return rng.standard_normal((sp["E"], sp["T"] + 1, z)).astype(np.float32), rng.standard_normal((sp["E"], sp["T"], z)).astype(np.float32)


def encoder_params():
    """The MlpVAE the cases run on (72 -> (36,) -> 8; the GPU tests' World.vae("mlp") builds the same one)."""
    rng = np.random.RandomState(21)
    p = vo.init_mlp_vae_params(3, z_dim=Z, source_shape=MLP_SRC, target_shape=MLP_SRC, encoder_sizes=MLP_ENC, decoder_sizes=(8,))
    for k in p:
        if k.endswith("bias"):
            p[k] = (0.05 * rng.standard_normal(p[k].shape)).astype(np.float32)
    return p


def encode(frames):
    """The encoder's mean of uint8 frames [n, ...] in float64, rounded to fp32: the latents a recording step leaves, up to its fp32 rounding."""
    frames = np.asarray(frames)
    with torch.no_grad():
        z = vo.mlp_vae_forward({k: torch.from_numpy(v).to(torch.float64) for k, v in encoder_params().items()}, frames.reshape(len(frames), -1).astype(np.float64) / 255.0, sample=False, dtype=torch.float64)["mean"]
    return z.numpy().astype(np.float32)


def frames_of(sp, sc):
    """The camera frames of a scripted collection: uint8 [E, T + 1, ...] and {(lane, slot): the final frame of a truncated step}, from the script's frame seed."""
    shape = MLP_SRC if sp["encoder"] == "mlp" else (80, 160, 3)
    rng = np.random.RandomState(sc["frame_seed"])
    frames = rng.randint(0, 256, (sp["E"], sp["T"] + 1) + shape, dtype=np.uint8)
    return frames, {(int(e), int(t)): rng.randint(0, 256, shape, dtype=np.uint8) for e, t in zip(*np.nonzero(sc["truncs"]))}


def encoder_latents(sp, cycle):
    """synthetic_latents' arrays from the encoder oracle on the script's frames (latents="encoder")."""
    assert sp["encoder"] == "mlp"
    sc = script(sp, cycle)
    frames, final = frames_of(sp, sc)
    E, T = sp["E"], sp["T"]
    lat = encode(frames.reshape((E * (T + 1),) + MLP_SRC)).reshape(E, T + 1, Z)
    fin = np.zeros((E, T, Z), np.float32)
    for (e, t), f in final.items():
        fin[e, t] = encode(f[None])[0]
    return lat, fin


def demo_script(sp):
    """The demonstrations of a case: uint8 frames [n, ...], measurements [n, 3] and expert actions [n, A] inside the action bounds (float32), seeded by the case."""
    n, A = sp["demo"]["n"], sp["A"]
    rng = np.random.RandomState(9000 * sp["seed"] + 7)
    frames = rng.randint(0, 256, (n,) + MLP_SRC, dtype=np.uint8)
    meas = np.stack([rng.uniform(-1, 1, n), rng.uniform(0, 1, n), rng.uniform(0, 2, n)], axis=1).astype(np.float32)
    low, high = bounds(A)
    return dict(frames=frames, meas=meas, actions=(low + (high - low) * rng.uniform(0.05, 0.95, (n, A))).astype(np.float32))


def given_observation_state(sp):
    """Case J's frozen observation statistics [count, mean, M2]: the moments of GIVEN_OBS_ROWS scripted rows [encoder latent | measurements] (a warm-up collection's)."""
    rng = np.random.RandomState(8000 * sp["seed"] + 3)
    n = GIVEN_OBS_ROWS
    lat = encode(rng.randint(0, 256, (n,) + MLP_SRC, dtype=np.uint8))
    meas = np.stack([rng.uniform(-1, 1, n), rng.uniform(0, 1, n), rng.uniform(0, 2, n)], axis=1).astype(np.float32)
    x = np.concatenate([lat, meas], axis=1).astype(np.float64)
    assert x.shape[1] == din_of(sp)
    return _merge([0.0, np.zeros(x.shape[1]), np.zeros(x.shape[1])], x)


# ------------------------------------------------------------------------------------------------------------------------------------ the trainer
def _merge(state, x):
    """Chan / Welford: the batch x [n, ...] (float64) into state = [count, mean, M2] -> the new state."""
    count, mean, m2 = state
    n_b = x.shape[0]
    if n_b == 0:
        return [count, mean, m2]
    m_b = x.sum(0) / n_b
    m2_b = ((x - m_b) ** 2).sum(0)
    delta, n_new = m_b - mean, count + n_b
    return [n_new, mean + delta * n_b / n_new, m2 + m2_b + delta ** 2 * count * n_b / n_new]


def _var(state):
    return state[2] / state[0] if state[0] > 0 else np.ones_like(np.asarray(state[2], np.float64))


def wave_sum(x):
    """The ordered fp64 sum of the finish kernels (include/mi355_carla.h: lane-strided partials and a wave reduction): lane l of 64 adds positions l, l + 64, .. from
    the first, then an xor tree over the lanes (offsets 32, 16, .. 1).  No fused multiply-add anywhere (the library is built with contraction off)."""
    x = np.asarray(x, np.float64)
    p = np.zeros(64)
    for t in range(len(x)):
        p[t % 64] = p[t % 64] + x[t]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[lanes ^ o]
    return float(p[0])


def normalise_ordered(a):
    """(a - mean) / (std + 1e-8) of one row or segment, population std, every sum a wave_sum: bit for bit what the finish kernels store."""
    a = np.asarray(a, np.float64)
    mean = wave_sum(a) / float(len(a))
    dd = a - mean
    sd = float(np.sqrt(wave_sum(dd * dd) / float(len(a))))
    return (a - mean) / (sd + 1e-8)


def normalised_bound(a, b, ddof=0):
    """What |da_i| <= b_i allows (a - mean) / (std + 1e-8) to differ by -> (per entry, the mean's bound, the std's bound).  |d mean| <= mean(b) = b_m; the std is the
    2-norm of the centred vector over sqrt(n - ddof), so |d std| <= sqrt(sum((b + b_m)^2) / (n - ddof)) = b_s; then
    |d a_n| <= (b + b_m) / (std + 1e-8) + |a_n| b_s / (std + 1e-8 - b_s).  One entry (or none the std divides by): exactly 0 on both sides."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = len(a)
    if n == 1 or n - ddof < 1:
        return np.zeros(n), float(b.mean()) if n else 0.0, 0.0
    sd = float(np.sqrt(((a - a.mean()) ** 2).sum() / (n - ddof))) + 1e-8
    b_m = float(b.mean())
    b_s = float(np.sqrt(((b + b_m) ** 2).sum() / (n - ddof)))
    return (b + b_m) / sd + np.abs((a - a.mean()) / sd) * b_s / max(sd - b_s, 1e-300), b_m, b_s


class Trainer:
    def __init__(self, sp, dtype=torch.float64, mutant=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.sp, self.dtype, self.mutant = sp, dtype, mutant
        self.ft = np.float64 if dtype == torch.float64 else np.float32
        self.on = set(sp["on"])
        self.low, self.high = bounds(sp["A"])
        self.params = OrderedDict((k, v.astype(self.ft)) for k, v in initial_params(sp).items())
        self.p0 = OrderedDict((k, v.astype(np.float64)) for k, v in self.params.items())
        self.adam = po.AdamTF(OrderedDict((k, v.shape) for k, v in self.params.items()), dtype=self.ft)
        self.episode = 0
        self.kl_coef = KL_COEF
        E, k, z = sp["E"], sp["k"], z_dim_of(sp)
        self.rs = [0.0, 0.0, 0.0]                                                    # reward scaling: count, mean, M2 of the discounted returns
        self.carry = np.zeros(E)
        self.obs = [0.0, np.zeros(din_of(sp)), np.zeros(din_of(sp))]                 # observation moments
        self.hist, self.fresh = np.zeros((E, max(k - 1, 0), z), np.float32), np.ones(E, bool)
        if sp["obs_given"]:
            self.obs = given_observation_state(sp)
        if sp["demo"] is not None:                                                   # the demonstration term: its coefficient, its own stream, [permutation, cursor]
            self.demo_coef, self.demo_rng, self.demo_state = float(sp["demo"]["coef"]), np.random.RandomState(sp["demo"]["seed"]), [None, 0]
        self.tol_m, self.tol_v, self.tol_acc = (OrderedDict((k, np.zeros(v.shape)) for k, v in self.params.items()) for _ in range(3))
        self.tol_s = 0.0

    # ---- pieces
    def propagate_gradient_tolerance(self, g, g_max, scale, rel_norm_tol, alpha):
        """What GRAD_TOL_X3 on every gradient lets one Adam step differ by, added per element into tol_acc ("THE bf16x3 PARAMETER BOUND" above).  g: the gradient
        Adam was given (clipped), g_max: max |g| per tensor in front of the clip factor `scale`, rel_norm_tol: the relative tolerance of the norm where the step
        was clipped; call behind adam.step."""
        b1, b2, eps = 0.9, 0.999, 1e-8
        self.tol_s = self.tol_s * b1 * b1 / b2 + (1 - b1) ** 2 / (1 - b2)
        cap = 2.0 * alpha * np.sqrt(self.tol_s)
        for k, v in g.items():
            a = GRAD_TOL_X3 * g_max[k] * scale + np.abs(v.astype(np.float64)) * rel_norm_tol
            self.tol_m[k] = self.tol_m[k] + (a - self.tol_m[k]) * (1 - b1)
            self.tol_v[k] = self.tol_v[k] + (a * a - self.tol_v[k]) * (1 - b2)
            sv, a_v = np.sqrt(self.adam.v[k].astype(np.float64)), np.sqrt(self.tol_v[k])
            rho = np.abs(self.adam.m[k].astype(np.float64)) / (sv + eps)
            lin = alpha * (self.tol_m[k] + rho * a_v) / (np.maximum(sv - a_v, 0.0) + eps)
            self.tol_acc[k] = self.tol_acc[k] + np.minimum(lin, cap)

    def lr(self):
        return np.float32(np.float32(self.sp["lr"]) * np.power(np.float32(HP["lr_decay"]), np.float32(self.episode)))

    def _tp(self, grad=False):
        return OrderedDict((k, torch.from_numpy(np.array(v)).to(self.dtype).requires_grad_(grad)) for k, v in self.params.items())

    def _t(self, x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(self.dtype)

    def assemble(self, col):
        """The stacked raw states of a collection [E, T + 1, din] float32 (NaN where no slot was written) from its latents; advances the history as the collection did."""
        sp = self.sp
        E, T, k = sp["E"], sp["T"], sp["k"]
        z, meas, lengths = col["latents"], col["meas"], col["lengths"]
        raw = np.full((E, T + 1, din_of(sp)), np.nan, np.float32)
        for e in range(E):
            n = int(lengths[e])
            for t in range(n + 1):
                boot = t == n
                done_last = n > 0 and (col["dones"][e, n - 1] or col["truncs"][e, n - 1])
                if boot and sp["kind"] == "continuous" and done_last:
                    break                                                            # a lane whose last step is a done or truncated takes no bootstrap
                if k == 1:
                    raw[e, t] = np.concatenate([z[e, t], meas[e, t]])
                    continue
                raw[e, t] = lc.stack_rows(self.hist, [e], [self.fresh[e]], z[e, t][None], meas[e, t][None])[0]
                if boot:
                    break                                                            # the bootstrap reads the history and does not advance it
                self.hist = lc.shift(self.hist, [e], [self.fresh[e]], z[e, t][None])
                self.fresh[e] = False
                if col["dones"][e, t] or (col["truncs"][e, t] and self.mutant != "truncation_keeps_history"):
                    self.fresh[e] = True
        return raw

    def peek(self, col):
        """(raw states, normalised states) of a collection as update() will see them, with nothing advanced: what the collection's actions and values are checked on."""
        hist, fresh = self.hist.copy(), self.fresh.copy()
        raw = self.assemble(col)
        self.hist, self.fresh = hist, fresh
        return raw, self.normalise(raw)[0]

    def obs_pair(self, state=None):
        state = self.obs if state is None else state
        return state[1], 1.0 / np.sqrt(_var(state) + STAT_EPS)

    def normalise(self, raw, state=None):
        """-> (the normalised states in this trainer's dtype, the values before the clamp in float64)."""
        if "observation_norm" not in self.on:
            return raw.astype(self.ft), None
        mean, inv = self.obs_pair(state)
        pre = (raw.astype(np.float64) - mean) * inv
        if self.ft == np.float32:                                                    # the fp32 pair; one subtract, one multiply
            n = (raw - mean.astype(np.float32)) * inv.astype(np.float32)
            return np.minimum(np.maximum(n, np.float32(-OBS_CLIP)), np.float32(OBS_CLIP)), pre
        return np.clip(pre, -OBS_CLIP, OBS_CLIP), pre

    def state_bound(self, raw, max_abs):
        """The bound of the module docstring on |device fp32 state - this float64 state|, per entry (0 where the reference clamps: equal there)."""
        mean, inv = self.obs_pair()
        x = raw.astype(np.float64)
        n = (x - mean) * inv
        b = U32 * (np.abs(mean) + np.abs(x - mean)) * inv + 2 * U32 * np.abs(n) + MOMENT_MEAN * max_abs * inv + MOMENT_VAR * np.abs(n)
        return np.where(np.abs(n) >= OBS_CLIP, 0.0, b)

    def predict(self, states, noise):
        """mean + sigma x noise clipped into the bounds, and the value, of every row."""
        with torch.no_grad():
            mean, ls, value = po.policy_forward(self._tp(), self._t(states), self.low, self.high)
            act = torch.clamp(mean + torch.exp(ls) * self._t(noise), self._t(self.low), self._t(self.high))
        return act.numpy().astype(np.float64), value.numpy().astype(np.float64)

    def segments(self, col, values=None, final_values=None):
        """(lane, first slot, length, bootstrap value) of every row / segment, lanes in order, slots ascending.  values / final_values: a refresh's tables in the
        place of the recorded ones."""
        sp, out = self.sp, []
        col = dict(col, values=col["values"] if values is None else values, final_values=col.get("final_values") if final_values is None else final_values)
        v = col["values"].astype(np.float64)
        for e in range(sp["E"]):
            n = int(col["lengths"][e])
            if n == 0:
                continue
            if sp["kind"] == "rollout":
                out.append((e, 0, n, v[e, n]))                                       # (a terminal masks it inside compute_gae)
                continue
            first = 0
            for t in range(n):
                if col["dones"][e, t] or col["truncs"][e, t] or t == n - 1:
                    boot = 0.0 if col["dones"][e, t] else float(col["final_values"][e, t]) if col["truncs"][e, t] else v[e, n]
                    out.append((e, first, t + 1 - first, boot))
                    first = t + 1
        return out

    def scale_rewards(self, col, frozen):
        """-> dict(G, scaled [E, T] NaN beyond a lane, den, pre: r / den before the clamp).  Advances the carries and (unless frozen) the moments."""
        sp = self.sp
        E, T = sp["E"], sp["T"]
        G = np.full((E, T), np.nan)
        for e in range(E):
            c = float(self.carry[e])
            for t in range(int(col["lengths"][e])):
                g = c * GAMMA
                g = g + float(col["rewards"][e, t])
                G[e, t] = g
                c = 0.0 if (col["dones"][e, t] or col["truncs"][e, t]) else g
            if col["lengths"][e] > 0:
                self.carry[e] = c
        rec = np.arange(T)[None, :] < col["lengths"][:, None]
        if not frozen:
            self.rs = [float(x) for x in _merge(self.rs, G[rec])]
        den = float(np.sqrt(_var(self.rs) + STAT_EPS))
        pre = np.where(rec, col["rewards"] / den, np.nan)
        return dict(G=G, den=den, pre=pre, scaled=np.clip(pre, -REWARD_CLIP, REWARD_CLIP), recorded=rec)

    def finish(self, col, rewards, values=None, final_values=None, weights=None, bars=None):
        """GAE, returns and the normalised advantages of every row / segment -> three [E, T] float64 arrays, NaN beyond a lane.  values [E, T + 1] / final_values
        [E, T]: a refresh's tables in the place of the recorded ones.  weights [E, T] with bars (rho_bar, c_bar): the V-trace finish of the header
        (mi_rollout_finish_vtrace: vtrace_cases.deltas / recurrence; RolloutBuffer by mi_rollout_finish's successor rule, the continuous buffer by the segment entries')."""
        sp = self.sp
        E, T = sp["E"], sp["T"]
        raw, ret, adv = (np.full((E, T), np.nan) for _ in range(3))
        v = (col["values"] if values is None else values).astype(np.float64)
        fv = col.get("final_values") if final_values is None else final_values
        c = dict(values=v, final_values=fv, dones=col["dones"].astype(np.float64), rewards=rewards, gamma=GAMMA)
        for e, first, n, boot in self.segments(col, values, final_values):
            sl = slice(first, first + n)
            if weights is None:
                a = po.compute_gae(rewards[e, sl], v[e, sl], boot, col["dones"][e, sl].astype(np.float64), GAMMA, LAM)
                raw[e, sl], ret[e, sl] = a, a + v[e, sl]
            else:
                kind = vc.TRUNCATED if col["truncs"][e, first + n - 1] else vc.OPEN
                D, a = vc.recurrence(vc.deltas(c, e, first, n, kind, sp["kind"] == "rollout"), weights[e, sl], GAMMA * LAM, bars[0], bars[1])
                raw[e, sl], ret[e, sl] = a, D + v[e, sl]
            adv[e, sl] = normalise_ordered(a)
        if sp["kind"] == "continuous" and sp["normalize"] == "batch":
            rec = ~np.isnan(raw)
            adv = np.where(rec, (raw - raw[rec].mean()) / (raw[rec].std() + 1e-8), np.nan)
        return raw, ret, adv

    def finish_bounds(self, col, rewards, values, final_values, weights, bars, b_values, b_final, b_weights, b_rewards):
        """What per-entry bounds on a refresh's inputs -- |dV| <= b_values [E, T + 1], |dV_final| <= b_final [E, T], |dw| <= b_weights [E, T] (None: GAE),
        |dr| <= b_rewards [E, T] -- allow its outputs to differ by: the finish's own linear recurrence run on the bounds, per segment -> (raw advantages, returns,
        normalised advantages), [E, T].  delta_t = r_t + g V_{t+1} - V_t gives b_delta = b_r + g b_V(t+1) + b_V(t) (g = 0 behind a terminal);
        D_t = gl c_t D_{t+1} + rho_t delta_t with c = min(c_bar, w), rho = min(rho_bar, w) gives b_D(t) = gl (c b_D(t+1) + b_c (|D_{t+1}| + b_D(t+1))) + rho b_delta +
        b_rho (|delta| + b_delta), where b_c / b_rho is the weight's bound below the bar and 0 above it (check_conditions keeps every weight RATIO_MARGIN from both
        bars); A_t = gl D_{t+1} + delta_t gives b_A = gl b_D(t+1) + b_delta; returns = D + V gives b_D + b_V.  GAE is the case w = 1, b_w = 0.  The normalisation
        (a - mean) / (std + 1e-8): |d mean| <= mean(b_A) = b_m, |d std| <= sqrt(mean((b_A + b_m)^2)) = b_s (the std is the 2-norm of the centred vector over sqrt n),
        so |d a_n| <= (b_A + b_m) / (std + 1e-8) + |a_n| b_s / max(std + 1e-8 - b_s, tiny); a one-step segment is exactly 0 on both sides."""
        sp = self.sp
        E, T = sp["E"], sp["T"]
        b_raw, b_ret, b_adv = (np.full((E, T), np.nan) for _ in range(3))
        v = values.astype(np.float64)
        raw, _, _ = self.finish(col, rewards, values, final_values, weights, bars)
        c = dict(values=v, final_values=final_values, dones=col["dones"].astype(np.float64), rewards=rewards, gamma=GAMMA)
        gl = GAMMA * LAM
        segs = self.segments(col, values, final_values)
        for e, first, n, _ in segs:
            last = first + n - 1
            trunc = bool(col["truncs"][e, last])
            kind = vc.TRUNCATED if trunc else vc.OPEN
            delta = vc.deltas(c, e, first, n, kind, sp["kind"] == "rollout")
            w = np.ones(n) if weights is None else weights[e, first:first + n]
            bw = np.zeros(n) if b_weights is None else b_weights[e, first:first + n]
            rho_bar, c_bar = (np.inf, np.inf) if bars is None else bars
            D_next, bD_next = 0.0, 0.0
            D = vc.recurrence(delta, w, gl, rho_bar, c_bar)[0]
            for i in range(n - 1, -1, -1):
                t = first + i
                done = bool(col["dones"][e, t])
                if i == n - 1:
                    b_succ = b_final[e, t] if trunc else 0.0 if done else b_values[e, t + 1]
                else:
                    b_succ = b_values[e, t + 1]
                b_delta = b_rewards[e, t] + (0.0 if done else GAMMA) * b_succ + b_values[e, t]
                cw, b_cw = (c_bar, 0.0) if w[i] > c_bar else (w[i], bw[i])
                rw, b_rw = (rho_bar, 0.0) if w[i] > rho_bar else (w[i], bw[i])
                b_raw[e, t] = gl * bD_next + b_delta
                bD = gl * (cw * bD_next + b_cw * (abs(D_next) + bD_next)) + rw * b_delta + b_rw * (abs(delta[i]) + b_delta)
                b_ret[e, t] = bD + b_values[e, t]
                D_next, bD_next = D[i], bD
        rec = ~np.isnan(raw)
        groups = [[(e, slice(first, first + n))] for e, first, n, _ in segs]
        if sp["kind"] == "continuous" and sp["normalize"] == "batch":
            groups = [[(e, slice(first, first + n)) for e, first, n, _ in segs]]
        for group in groups:
            a = np.concatenate([raw[e, sl] for e, sl in group])
            b = np.concatenate([b_raw[e, sl] for e, sl in group])
            out = normalised_bound(a, b)[0]
            i = 0
            for e, sl in group:
                k = sl.stop - sl.start
                b_adv[e, sl] = out[i:i + k]
                i += k
        assert np.array_equal(np.isnan(b_raw), ~rec)
        return b_raw, b_ret, b_adv

    def refresh(self, col, states, raw_states, rewards, a_all, logp_old, ve, vt):
        """A refresh (advantage recomputation) under the current parameters: the values of every recorded row and bootstrap slot of `states`, in the continuous buffer
        also of the truncated steps' final observations (col["final_states"], data), each rounded to fp32 (the tables values_now / final_values_now); with V-trace
        the weights w = exp(log pi_theta - log pi_old) of every recorded step from the two fp32 tables; then the finish again on the rewards the first finish read
        -> dict(values [E, T + 1], final [E, T] or None, weights [E, T] or None, raw, ret, adv, and in the float64 reference the per-entry bounds b_*)."""
        sp, mutant = self.sp, self.mutant
        E, T = sp["E"], sp["T"]
        lengths = np.asarray(col["lengths"])
        src = raw_states if mutant == "refresh_values_raw_states" else states
        slots = ~np.isnan(raw_states).any(-1)                                        # every recorded row and every bootstrap slot that was recorded
        if mutant == "stale_bootstrap_slots":
            slots = slots & (np.arange(T + 1)[None, :] < lengths[:, None])
        p = self._tp()
        values = col["values"].astype(np.float32).copy()                             # (values_now starts as a copy of values)
        with torch.no_grad():
            values[slots] = po.policy_forward(p, self._t(src[slots]), self.low, self.high)[2].numpy().astype(np.float32)
        b_values = ar.ABS + ar.REL * np.abs(values.astype(np.float64))
        final = b_final = None
        if sp["kind"] == "continuous":
            final = np.asarray(col["final_values"], np.float32).copy()
            cut = np.nonzero(col["truncs"])
            if len(cut[0]) and mutant != "refresh_bootstraps_from_recorded_final_values":
                with torch.no_grad():
                    final[cut] = po.policy_forward(p, self._t(col["final_states"][cut]), self.low, self.high)[2].numpy().astype(np.float32)
            b_final = ar.ABS + ar.REL * np.abs(np.nan_to_num(final.astype(np.float64)))
        weights = b_weights = bars = None
        out = {}
        if sp["vtrace"] is not None:
            bars = tuple(reversed(sp["vtrace"])) if mutant == "vtrace_bars_swapped" else tuple(sp["vtrace"])
            with torch.no_grad():
                mean, ls, _ = po.policy_forward(p, self._t(src[ve, vt]), self.low, self.high)
                lp_now = po.normal_log_prob(a_all, mean, ls).sum(-1)
            z = ((a_all - mean) / torch.exp(ls)).numpy().astype(np.float64)
            terms = (0.5 * z * z + np.abs(ls.numpy().astype(np.float64)) + po.HALF_LOG_2PI).sum(-1)      # the absolute terms of log pi_theta
            if mutant == "refresh_recaches_logp_old":
                logp_old = dict(logp_old, table=lp_now.numpy().astype(np.float32))
            d = lp_now.numpy().astype(np.float32).astype(np.float64) - logp_old["table"].astype(np.float64)      # two fp32 tables
            weights, b_weights = np.full((E, T), np.nan), np.full((E, T), np.nan)
            weights[ve, vt] = np.exp(d)
            b_weights[ve, vt] = weights[ve, vt] * np.expm1(LOGP_REL * terms + LOGP_REL * logp_old["terms"])
            out["logp_now"] = lp_now
        raw, ret, adv = self.finish(col, rewards, values, final, weights, bars)
        out.update(values=values, final=final, weights=weights, bars=bars, raw=raw, ret=ret, adv=adv)
        if self.ft == np.float64 and mutant is None:
            rec = ~np.isnan(raw)
            r_abs = np.abs(np.nan_to_num(rewards))                                   # the scaled rewards' own row of compare(): 1e-9 relative and an fp64 ulp
            b_rewards = np.where(rec, MOMENT_VAR * r_abs + np.spacing(r_abs), 0.0) if "reward_scaling" in self.on else np.zeros((E, T))
            out["b_raw"], out["b_ret"], out["b_adv"] = self.finish_bounds(col, rewards, values, final, weights, bars, b_values, b_final, b_weights, b_rewards)
            out["b_weights"] = b_weights
        return out

    def losses(self, p, s, a, R, adv, logp_old, mean_old, lso, v_old, beta, demo=None):
        """The loss terms of one minibatch as torch scalars, and what the conditions read.  demo: None or dict(s, a: the step's demonstration rows and the expert's
        actions, coef, kind): loss = L_ppo(PPO rows) + float32(coef) x clone_loss(demonstration rows) (demo_term_cases.demo_terms, 1 / M_demo); every other term
        stays a mean over the PPO rows."""
        hp = HP
        share = 1.0
        if demo is not None and self.mutant == "penalty_and_value_terms_over_demo_rows":      # the value term and the penalty as means over M + M_demo rows
            share = len(s) / float(len(s) + len(demo["s"]))
        mean, ls, value = po.policy_forward(p, s, self.low, self.high)
        logp = po.normal_log_prob(a, mean, ls).sum(-1)
        ratio = torch.exp(logp - logp_old)
        pl = torch.minimum(ratio * adv, torch.clamp(ratio, 1.0 - hp["epsilon"], 1.0 + hp["epsilon"]) * adv).mean()
        l_u = (value - R) ** 2
        if v_old is None:
            vl = l_u.mean() * hp["value_scale"]
        else:
            v_c = torch.minimum(torch.maximum(value, v_old - VALUE_CLIP), v_old + VALUE_CLIP)
            vl = torch.maximum(l_u, (v_c - R) ** 2).mean() * hp["value_scale"]
        vl = vl * share
        el = (0.5 + po.HALF_LOG_2PI + ls).sum() * hp["entropy_scale"]
        out = dict(policy_loss=pl, value_loss=vl, entropy_loss=el, ratio=ratio, value=value, mean=mean)
        loss = -pl + vl - el
        if demo is not None:
            mean_d = po.policy_forward(p, demo["s"], self.low, self.high)[0]
            dl = dc.demo_terms(mean_d, demo["a"], ls, demo["kind"]).mean()
            z = ((demo["a"] - mean_d) / torch.exp(ls)).detach()
            out["demo_loss"], out["mean_sq_error"] = dl, ((mean_d - demo["a"]) ** 2).sum(-1).mean()
            out["demo_abs_terms"] = (0.5 * z * z + ls.detach().abs() + po.HALF_LOG_2PI).sum(-1).mean() if demo["kind"] == "nll" else dl.detach()
            loss = loss + torch.tensor(float(np.float32(demo["coef"])), dtype=self.dtype) * dl
        if beta is not None:
            d, D = ls - lso, mean - mean_old
            kl = (d + 0.5 * torch.expm1(-2.0 * d) + D * D / (2.0 * torch.exp(2.0 * ls))).sum(-1).mean() * share
            out["kl"], out["penalty"] = kl, torch.tensor(float(np.float32(beta)), dtype=self.dtype) * kl
            if self.mutant != "penalty_behind_clip":
                loss = loss + out["penalty"]
        out["loss"] = loss
        return out

    def update(self, col, frozen=False, target_kl=None, diagnostics=None):
        """One cycle (see the module docstring) -> the keys of update() / update_with_diagnostics(), `params` (float64 copies), `raw_states`, `states` and
        `margins` (what the conditions are checked on).  Draws from the legacy numpy stream as the update does: seed it first."""
        sp, on, ft, hp, mutant = self.sp, self.on, self.ft, HP, self.mutant
        E, T, A, batch = sp["E"], sp["T"], sp["A"], sp["batch"]
        diagnostics = sp["diagnostics"] if diagnostics is None else diagnostics
        out, mg = {}, dict(ratio=[], value=[], norm=[], kl_stop=[])
        lengths = np.asarray(col["lengths"], np.int32)
        rec = np.arange(T)[None, :] < lengths[:, None]
        valid = [(e, t) for e in range(E) for t in range(int(lengths[e]))]
        ve, vt = np.array([e for e, _ in valid]), np.array([t for _, t in valid])
        n_valid = len(valid)
        raw_states = self.assemble(col)
        # ---- rewards, finish
        rewards = np.where(rec, col["rewards"], np.nan)
        if "reward_scaling" in on:
            sr = self.scale_rewards(col, frozen)
            out.update(return_rms=dict(count=self.rs[0], mean=self.rs[1], var=float(_var(self.rs))), reward_scale_den=sr["den"], discounted_returns=sr["G"],
                       scaled_rewards=sr["scaled"], reward_clip_fraction=float((np.abs(sr["scaled"][rec]) == REWARD_CLIP).mean()), return_carry=self.carry.copy())
            mg["reward_pre"] = sr["pre"][rec]
            read = col["rewards"] if mutant == "finish_reads_unscaled_rewards" else sr["scaled"]
        else:
            read = col["rewards"]
        read_tab = np.where(rec, read, np.nan)
        raw_adv, returns, adv = self.finish(col, read_tab)
        out.update(lengths=lengths, raw_advantages=raw_adv, returns=returns, advantages=adv, samples=n_valid, segment_list=[s[:3] for s in self.segments(col)])
        ret_tab = returns
        if mutant == "returns_of_unscaled_rewards":
            ret_tab = self.finish(col, rewards)[1]
        # ---- the states the policy acted on
        obs_state = self.obs
        raw_valid = raw_states[ve, vt]
        obs_frozen = frozen or sp["obs_given"]                                       # (given statistics are frozen in every cycle)
        if mutant == "observation_merge_before_epochs" and "observation_norm" in on and not obs_frozen:
            obs_state = _merge(self.obs, raw_valid.astype(np.float64))
        states, pre = self.normalise(raw_states, obs_state)
        out["raw_states"], out["states"] = raw_states, states
        self.x_max = max(getattr(self, "x_max", 0.0), float(np.abs(raw_valid).max()))
        out["state_bound"] = self.state_bound(raw_states, self.x_max) if pre is not None else np.zeros(raw_states.shape)
        if pre is not None:
            mg["obs_pre"] = pre[ve, vt]
            before = (np.abs(np.clip(pre[ve, vt], -OBS_CLIP, OBS_CLIP)) == OBS_CLIP)
            out["observation_clip_fraction"] = before.sum(0) / n_valid
        s_all = self._t(states[ve, vt])
        a_all = self._t(col["actions"][ve, vt])
        R_all = self._t(ret_tab[ve, vt].astype(np.float32))
        v_old_all = self._t(col["values"][ve, vt]) if "value_clip" in on else None
        adv_seg = adv[ve, vt].astype(np.float32)
        # ---- the old policy
        old = self._tp()
        with torch.no_grad():
            s_old = self._t(raw_valid) if mutant == "old_policy_on_raw_states" else s_all
            mean_old, lso, _ = po.policy_forward(old, s_old, self.low, self.high)
            logp_old = po.normal_log_prob(a_all, mean_old, lso).sum(-1)
        out["logp_old_max"] = float(logp_old.abs().max())
        beta = self.kl_coef if "kl_penalty" in on else None
        # ---- the newer settings: what a refresh reads of the old policy (the update's ONE cache of log pi_old, an fp32 table) and the demonstration rows
        recompute, demo = sp["recompute"], sp["demo"]
        z_old = ((a_all - mean_old) / torch.exp(lso)).numpy().astype(np.float64)
        cache = dict(table=logp_old.numpy().astype(np.float32), terms=(0.5 * z_old * z_old + np.abs(lso.numpy().astype(np.float64)) + po.HALF_LOG_2PI).sum(-1))
        raw_cur, R_first, rf, refreshes, recomputed = raw_adv, R_all, None, [], 0
        if demo is not None:
            d_s, d_a, n_demo = self._t(col["demo_states"]), self._t(col["demo_actions"]), len(col["demo_states"])
            demo_recs, demo_rows = [], []
        # ---- the epochs
        recs, norms, scales, norm_tols, mb_stats, epochs, stopped = [], [], [], [], [], [], False
        mb_adv = np.full((E, T), np.nan, np.float32)
        mb_tols, mb_adv_tol = [], np.zeros((E, T))
        first_step = [0]
        def refreshed():
            """One refresh: from here on the steps, the minibatch normalisation and the diagnostics read its tables (fp32 where the device's table is)."""
            read = np.where(rec, col["rewards"], np.nan) if mutant == "refresh_reads_unscaled_rewards" else read_tab
            r = self.refresh(col, states, raw_states, read, a_all, cache, ve, vt)
            if r["weights"] is not None:
                w = r["weights"][ve, vt]
                mg["vtrace"].append(np.minimum(np.abs(w - r["bars"][0]), np.abs(w - r["bars"][1])))
            return r
        mg["vtrace"] = []
        for epoch in range(sp["epochs"]):
            if recompute and mutant != "no_refresh" and (epoch > 0 or mutant == "refresh_before_epoch_1"):
                rf = refreshed()
                refreshes.append(rf)
                recomputed += 1
                R_all, adv_seg = self._t(rf["ret"][ve, vt].astype(np.float32)), rf["adv"][ve, vt].astype(np.float32)
                if mutant != "minibatch_norm_reads_first_raw_advantages":
                    raw_cur = rf["raw"]
                if mutant == "value_clip_reads_refreshed_values" and v_old_all is not None:
                    v_old_all = self._t(rf["values"][ve, vt])
                if mutant == "refresh_recaches_logp_old" and "logp_now" in rf:
                    logp_old = rf["logp_now"]
                    cache = dict(cache, table=logp_old.numpy().astype(np.float32))
            order = np.arange(n_valid)
            np.random.shuffle(order)
            for i in range(0, n_valid, batch):
                mb = order[i:i + batch]
                if "minibatch_norm" in on:
                    a_in = (adv[ve, vt] if mutant == "minibatch_norm_of_normalised" else raw_cur[ve, vt])[mb]
                    mean = a_in.sum() / len(mb)
                    ss = ((a_in - mean) ** 2).sum()
                    std = float(np.sqrt(ss / (len(mb) - sp["ddof"]))) if len(mb) - sp["ddof"] >= 1 else 0.0
                    a_mb = ((a_in - mean) / (std + 1e-8)).astype(np.float32)
                    mb_stats.append((float(len(mb)), float(mean), std))
                    mb_adv[ve[mb], vt[mb]] = a_mb
                    if rf is not None and "b_raw" in rf and raw_cur is rf["raw"]:     # behind a refresh the raw advantages carry its per-entry bounds
                        b_mb, b_m, b_s = normalised_bound(a_in, rf["b_raw"][ve, vt][mb], sp["ddof"])
                        mb_tols.append((b_m, b_s))
                        mb_adv_tol[ve[mb], vt[mb]] = b_mb
                    else:
                        mb_tols.append((0.0, 0.0))
                else:
                    a_mb = adv_seg[mb]
                p = self._tp(grad=True)
                idx = torch.from_numpy(mb)
                v_old = None if v_old_all is None else v_old_all[idx]
                d_kw = None
                if demo is not None:                                                 # min(batch_size, n) rows by the documented rule, from the setting's own stream
                    rows = dc.demonstration_rows(np.random if mutant == "demo_rows_from_the_legacy_stream" else self.demo_rng, self.demo_state, n_demo, demo["batch"], 1)[0]
                    mg.setdefault("demo_redraws", []).append(np.array([float(len(demo_rows) > 0 and self.demo_state[1] == len(rows))]))      # a fresh permutation behind the update's first step
                    demo_rows.append(rows)
                    d_idx = torch.from_numpy(rows.astype(np.int64))
                    d_kw = dict(s=d_s[d_idx], a=d_a[d_idx], coef=self.demo_coef, kind=demo["loss"])
                L = self.losses(p, s_all[idx], a_all[idx], R_all[idx], self._t(a_mb), logp_old[idx], mean_old[idx], lso, v_old, beta, d_kw)
                L["loss"].backward()
                g = OrderedDict((k, (v.grad if v.grad is not None else torch.zeros_like(v)).numpy().astype(ft)) for k, v in p.items())
                L = {k: v.detach() for k, v in L.items()}
                r = dict(policy_loss=float(L["policy_loss"]), value_loss=float(L["value_loss"]), entropy_loss=float(L["entropy_loss"]), prob_ratio=float(L["ratio"].mean()))
                r["loss"] = float(L["loss"])
                if demo is not None:
                    demo_recs.append(dict(demo_loss=float(L["demo_loss"]), mean_sq_error=float(L["mean_sq_error"]), abs_terms=float(L["demo_abs_terms"])))
                if beta is not None:
                    r["kl"], r["kl_penalty"] = float(L["kl"]), float(L["penalty"])
                    klm, _, mag = kc.kl_terms(L["mean"].numpy(), mean_old[idx].numpy(), p["policy/action_logstd"].detach().numpy(), lso.numpy())
                    r["kl_bound"] = kc.kl_bound(float(klm.mean()), float(mag.mean()))
                    r["kl_floor_share"] = kc.KL_FLOOR_ULP * float(mag.mean()) / r["kl_bound"]
                    if mutant == "penalty_behind_clip":
                        r["loss"] += r["kl_penalty"]
                recs.append(r)
                ratio = L["ratio"].numpy().astype(np.float64)
                mg["ratio"].append(np.minimum(np.abs(ratio - (1 - hp["epsilon"])), np.abs(ratio - (1 + hp["epsilon"]))))
                if v_old_all is not None:
                    dv = (L["value"] - v_old_all[idx]).numpy().astype(np.float64)
                    mg["value"].append(np.abs(np.abs(dv) - VALUE_CLIP))
                if "grad_clip" in on:
                    norm = float(np.sqrt(sum((v.astype(np.float64) ** 2).sum() for v in g.values())))
                    c = sp["max_grad_norm"]
                    scale = np.float32(c / norm) if norm > c else np.float32(1.0)
                    norms.append(norm)
                    scales.append(float(scale))
                    mg["norm"].append(abs(norm - c) / c)
                    norm_tols.append(GRAD_TOL_X3 * float(np.sqrt(sum(v.size * float(np.abs(v).max()) ** 2 for v in g.values()))))
                    g_max = {k: float(np.abs(v).max()) for k, v in g.items()}
                    g = OrderedDict((k, (v * ft(scale)).astype(ft)) for k, v in g.items())
                if mutant == "penalty_behind_clip" and beta is not None:            # the penalty's gradient added behind the clip factor
                    p2 = self._tp(grad=True)
                    L2 = self.losses(p2, s_all[idx], a_all[idx], R_all[idx], self._t(a_mb), logp_old[idx], mean_old[idx], lso, None, beta)
                    L2["penalty"].backward()
                    g = OrderedDict((k, (v + (p2[k].grad.numpy().astype(ft) if p2[k].grad is not None else 0)).astype(ft)) for k, v in g.items())
                alpha = float(self.adam.alpha(self.lr()))
                self.adam.step(self.params, g, self.lr())
                if ft == np.float64 and "grad_clip" in on and mutant is None:
                    self.propagate_gradient_tolerance(g, g_max, float(scale), norm_tols[-1] / norm if scale < 1.0 else 0.0, alpha)
            first_step.append(len(recs))
            if diagnostics:
                ep = self.observe(s_all, a_all, R_first if mutant == "diagnostics_read_first_returns" else R_all, logp_old, v_old_all, mg)
                if "grad_clip" in on:
                    lo, hi = first_step[-2], first_step[-1]
                    ep["grad_norm_max"], ep["clipped_steps"] = float(max(norms[lo:hi])), int(sum(s < 1.0 for s in scales[lo:hi]))
                epochs.append(ep)
                if target_kl is not None:
                    mg["kl_stop"].append(abs(ep["approx_kl"] - target_kl) / target_kl)
                    if ep["approx_kl"] > target_kl:
                        stopped = True
                        if mutant == "refresh_behind_the_kl_stop" and recompute and epoch + 1 < sp["epochs"]:
                            rf = refreshed()
                            recomputed += 1
                        break
        out["losses"] = recs
        if recompute:                                                                # the keys of advantage recomputation and V-trace: the LAST refresh that ran
            out["recomputed_epochs"] = recomputed
            if rf is not None:
                out.update(refreshed_values=np.where(rec, rf["values"][:, :T], np.float32(np.nan)).astype(np.float32), refreshed_returns=rf["ret"],
                           refreshed_advantages=rf["adv"], refreshed_raw_advantages=rf["raw"])
                if sp["kind"] == "continuous":
                    out["refreshed_final_values"] = np.where(col["truncs"], rf["final"], np.float32(np.nan)).astype(np.float32)
                if rf["weights"] is not None:
                    w = rf["weights"][rec]
                    out.update(refreshed_importance_weights=rf["weights"], vtrace_rho_clip_fraction=float((w > rf["bars"][0]).mean()),
                               vtrace_c_clip_fraction=float((w > rf["bars"][1]).mean()))
                out["refresh_bounds"] = {k: rf[k] for k in ("b_raw", "b_ret", "b_adv", "b_weights") if rf.get(k) is not None}
                out["refresh_moved"] = dict(values=np.abs(rf["values"][:, :T].astype(np.float64) - col["values"][:, :T].astype(np.float64)),
                                            final=None if rf["final"] is None else np.abs(rf["final"].astype(np.float64) - np.asarray(col["final_values"], np.float64)))
            if mutant == "result_returns_are_refreshed" and rf is not None:
                out.update(returns=rf["ret"], advantages=rf["adv"], raw_advantages=rf["raw"])
        if demo is not None:
            out.update(demo_losses=demo_recs, demo_rows=demo_rows, demo_coef=float(self.demo_coef), demo_coef_next=float(self.demo_coef * demo["decay"]))
            if mutant != "demo_coef_next_unused":
                self.demo_coef = out["demo_coef_next"]
        if "grad_clip" in on:
            out["grad_norms"], out["clip_scales"], out["grad_norm_tols"] = np.array(norms), np.array(scales), np.array(norm_tols)
            out["param_tols"] = OrderedDict((k, float(np.sqrt(np.mean(v ** 2)))) for k, v in self.tol_acc.items())
        if diagnostics:
            out.update(epochs=epochs, epochs_run=len(epochs), stopped_early=stopped)
        if "minibatch_norm" in on:
            out["minibatch_adv_stats"], out["minibatch_advantages"] = np.array(mb_stats).reshape(-1, 3), mb_adv
            if recompute:
                out["minibatch_stat_tols"], out["minibatch_advantages_tol"] = np.array(mb_tols).reshape(-1, 2), mb_adv_tol
        # ---- behind the last epoch
        if beta is not None:
            with torch.no_grad():
                mean, ls, _ = po.policy_forward(self._tp(), s_all, self.low, self.high)
            klm, part, mag = kc.kl_terms(mean.numpy(), mean_old.numpy(), ls.numpy(), lso.numpy())
            kl = float(klm.mean())
            out["kl"] = dict(samples=n_valid, kl=kl, kl_std=float(np.sqrt(max((klm ** 2).mean() - kl * kl, 0.0))), kl_mean_part=float(part.mean()))
            out["kl_floor_share"] = kc.KL_FLOOR_ULP * float(mag.mean()) / kc.kl_bound(kl, float(mag.mean()))
            out["kl_coef"], out["kl_adapted"] = float(self.kl_coef), True
            out["kl_coef_next"] = float(kc.adapted(self.kl_coef, KL_TARGET, kl))
            if mutant != "kl_coef_next_unused":
                self.kl_coef = out["kl_coef_next"]
        if "observation_norm" in on:                                                  # the merge stands behind the epochs: this update ran on the moments as they were
            if not obs_frozen:
                self.obs = obs_state if mutant == "observation_merge_before_epochs" else _merge(self.obs, raw_valid.astype(np.float64))
                if mutant == "observation_merge_twice":
                    self.obs = _merge(self.obs, raw_valid.astype(np.float64))
            out["observation_rms"] = dict(count=float(self.obs[0]), mean=self.obs[1].copy(), var=_var(self.obs))
        out["params"], out["p0"] = OrderedDict((k, v.astype(np.float64)) for k, v in self.params.items()), self.p0
        out["margins"] = {k: (np.concatenate([np.ravel(x) for x in v]) if len(v) else np.zeros(0)) if isinstance(v, list) else np.ravel(v) for k, v in mg.items()}
        return out

    def observe(self, s, a, R, logp_old, v_old, mg):
        """The diagnostics of one epoch over all valid rows under the current parameters (sums in float64)."""
        hp = HP
        with torch.no_grad():
            mean, ls, value = po.policy_forward(self._tp(), s, self.low, self.high)
            lp = po.normal_log_prob(a, mean, ls).sum(-1)
        d = (lp - logp_old).numpy().astype(np.float64)
        r, v, ret = np.exp(d), value.numpy().astype(np.float64), R.numpy().astype(np.float64)
        err = ret - v
        mg["ratio"].append(np.minimum(np.abs(r - (1 - hp["epsilon"])), np.abs(r - (1 + hp["epsilon"]))))
        ep = dict(samples=len(d), approx_kl=float((r - 1 - d).mean()), approx_kl_k1=float(-d.mean()), clip_fraction=float((np.abs(r - 1) > hp["epsilon"]).mean()),
                  ratio_mean=float(r.mean()), value_mse=float((err ** 2).mean()), explained_variance=float(1.0 - err.var() / ret.var()))
        if v_old is not None:
            vo = v_old.numpy().astype(np.float64)
            l_u, l_c = (v - ret) ** 2, (np.clip(v, vo - VALUE_CLIP, vo + VALUE_CLIP) - ret) ** 2
            mg["value"].append(np.abs(np.abs(v - vo) - VALUE_CLIP))
            ep.update(value_clip_fraction=float((np.abs(v - vo) > VALUE_CLIP).mean()), value_loss_clipped=float(np.maximum(l_u, l_c).mean()),
                      value_grad_zero_fraction=float((l_c > l_u).mean()))
        return ep


# ------------------------------------------------------------------------------------------------------------------------------------ host-side collections
def synthetic_collection(tr, sp, cycle):
    """A collection without a device: the script's observations on synthetic latents, the actions and values of `tr`'s own float64 forward rounded to fp32 (what a
    recording step leaves), final_values of the truncated steps likewise.  Does NOT advance tr's history (a copy assembles)."""
    sc = script(sp, cycle)
    lat, fin = synthetic_latents(sp, cycle) if sp["latents"] == "synthetic" else encoder_latents(sp, cycle)
    lengths = lengths_of(sp, sc)
    col = dict(latents=lat, meas=sc["meas"], rewards=sc["rewards"], dones=sc["dones"], truncs=sc["truncs"], lengths=lengths, noise=sc["noise"])
    hist, fresh = tr.hist.copy(), tr.fresh.copy()
    raw = tr.assemble(col)
    states, _ = tr.normalise(np.nan_to_num(raw))
    E, T, A = sp["E"], sp["T"], sp["A"]
    noise = np.concatenate([sc["noise"], np.zeros((E, 1, A), np.float32)], axis=1)   # (slot T: a bootstrap, greedy)
    acts, vals = tr.predict(states.reshape(E * (T + 1), -1), noise.reshape(E * (T + 1), A))
    col["actions"], col["values"] = acts.reshape(E, T + 1, A).astype(np.float32), vals.reshape(E, T + 1).astype(np.float32)
    fv = np.full((E, T), np.nan, np.float32)
    fs = np.full((E, T, din_of(sp)), np.nan, np.float32)                            # final_states: the truncated steps' final observations as state rows (fp32 table)
    h2, f2 = hist.copy(), fresh.copy()
    for e, t in zip(*np.nonzero(sc["dones"] | sc["truncs"] | True)):                # lane by lane, slots ascending: the history as the collection saw it
        if t >= lengths[e]:
            continue
        if sp["k"] > 1:
            h2 = lc.shift(h2, [e], [f2[e]], lat[e, t][None])
            f2[e] = False
        if sc["truncs"][e, t]:                                                       # valued on the stopped episode's history: the row a step of the final observation would assemble
            frow = np.concatenate([fin[e, t], sc["final_meas"][e, t]])
            if sp["k"] > 1:
                frow = lc.stack_rows(h2, [e], [f2[e]], fin[e, t][None], sc["final_meas"][e, t][None])[0]
            fs[e, t] = tr.normalise(frow[None])[0][0].astype(np.float32)
            fv[e, t] = tr.predict(tr.normalise(frow[None])[0], np.zeros((1, A), np.float32))[1][0]
        if sc["dones"][e, t] or sc["truncs"][e, t]:
            f2[e] = True
    col["final_values"], col["final_states"] = fv, fs
    if sp["demo"] is not None:                                                       # the demonstration tables as DemonstrationBuffer.add leaves them: normalised fp32 rows, the expert's actions
        ds = demo_script(sp)
        rows = np.concatenate([encode(ds["frames"]), ds["meas"]], axis=1).astype(np.float32)
        col["demo_states"], col["demo_actions"] = tr.normalise(rows)[0].astype(np.float32), ds["actions"]
    tr.hist, tr.fresh = hist, fresh
    return col


def run_host(name, dtype=torch.float64, mutant=None, seed=5, feed=None):
    """Every cycle of a case on synthetic collections -> (the list of update results, the trainer).  The collections are made by a float64 trainer WITHOUT the mutant
    (what the device does), so that a mutant changes the update and nothing else; feed: that list of collections, to save making them again."""
    sp = spec(name)
    tr = Trainer(sp, dtype, mutant)
    maker = Trainer(sp) if feed is None else None
    outs, cols = [], []
    for cycle, frozen in enumerate(sp["cycles"]):
        col = synthetic_collection(maker, sp, cycle) if feed is None else feed[cycle]
        cols.append(col)
        target = case_target_kl(name, col) if sp["target_kl"] is not None else None
        np.random.seed(seed + cycle)
        outs.append(tr.update(col, frozen=frozen, target_kl=target))
        tr.episode += 1
        if maker is not None:
            np.random.seed(seed + cycle)
            maker.update(col, frozen=frozen, target_kl=target)
            maker.episode += 1
    return outs, tr, cols


_TARGETS = {}


def case_target_kl(name, col, seed=5):
    """Case F: the geometric mean of the float64 reference's epoch-1 and epoch-2 k3 on this collection (no stop), so that the stop fires behind epoch 2."""
    key = (name, float(np.asarray(col["values"], np.float64).sum()))
    if key not in _TARGETS:
        np.random.seed(seed)
        ep = Trainer(spec(name)).update(col, target_kl=None, diagnostics=True)["epochs"]
        _TARGETS[key] = (float(np.sqrt(ep[0]["approx_kl"] * ep[1]["approx_kl"])), ep[0]["approx_kl"], ep[1]["approx_kl"])
    return _TARGETS[key][0]


def case_f_k3(name, col):
    """(the target, the reference's epoch-1 k3, its epoch-2 k3) of case_target_kl."""
    case_target_kl(name, col)
    return _TARGETS[(name, float(np.asarray(col["values"], np.float64).sum()))]


def trajectory_errors(p_dev, p_twin, p_ref, p0):
    """tests/test_c_c3_ppo_gpu.py's rule per tensor -> [(name, device RMS error, twin RMS error, max |update|)] against the float64 trajectory."""
    rows = []
    for k in p_ref:
        upd = p_ref[k] - p0[k]
        e_d = float(np.sqrt(np.mean(((np.asarray(p_dev[k], np.float64) - p0[k]) - upd) ** 2)))
        e_t = float(np.sqrt(np.mean(((np.asarray(p_twin[k], np.float64) - p0[k]) - upd) ** 2)))
        rows.append((k, e_d, e_t, float(max(np.abs(upd).max(), 1e-12))))
    return rows


def check_conditions(name, outs):
    """The conditions the exact counts and the relative bounds rest on, on the float64 results of a case -> a dict of the figures; raises AssertionError with
    the figure that misses."""
    sp = spec(name)
    fig = dict(ratio_gap=min(o["margins"]["ratio"].min() for o in outs))
    assert fig["ratio_gap"] >= RATIO_MARGIN, (name, "ratio", fig)
    if "value_clip" in sp["on"]:
        fig["value_gap"] = min(o["margins"]["value"].min() for o in outs)
        assert fig["value_gap"] >= VALUE_MARGIN, (name, "value", fig)
    if "reward_scaling" in sp["on"]:
        pre = np.concatenate([o["margins"]["reward_pre"] for o in outs])
        fig["reward_gap"] = float(np.abs(np.abs(pre) / REWARD_CLIP - 1).min())
        fig["reward_clamped"] = int((np.abs(pre) > REWARD_CLIP).sum())
        assert fig["reward_gap"] >= CLAMP_MARGIN and fig["reward_clamped"] >= 1, (name, "reward clamp", fig)
    if "observation_norm" in sp["on"]:
        pre = np.concatenate([o["margins"]["obs_pre"].ravel() for o in outs])
        fig["obs_gap"] = float(np.abs(np.abs(pre) / OBS_CLIP - 1).min())
        fig["obs_clamped"] = int((np.abs(pre) > OBS_CLIP).sum())
        assert fig["obs_gap"] >= CLAMP_MARGIN and fig["obs_clamped"] >= 1, (name, "observation clamp", fig)
    if "grad_clip" in sp["on"]:
        scales = np.concatenate([o["clip_scales"] for o in outs])
        fig["norm_gap"] = min(o["margins"]["norm"].min() for o in outs)
        fig["clipped"], fig["unclipped"] = int((scales < 1).sum()), int((scales == 1).sum())
        assert fig["norm_gap"] >= NORM_MARGIN and fig["clipped"] >= 1 and fig["unclipped"] >= 1, (name, "gradient clipping", fig)
    if "kl_penalty" in sp["on"]:
        fig["kl_end"] = [o["kl"]["kl"] for o in outs]
        fig["kl_floor_share"] = [o["kl_floor_share"] for o in outs]
        assert min(fig["kl_end"]) >= KL_MIN, (name, "KL magnitude", fig)
        if sp["kl_share_max"] is not None:                                           # the KL case: the floor is at most 10 % of kl_bound at the end of the cycle and
            fig["kl_floor_share_steps"] = [l["kl_floor_share"] for o in outs for l in o["losses"][1:]]      # at every step behind the first (whose KL is exactly 0)
            assert max(fig["kl_floor_share"] + fig["kl_floor_share_steps"]) <= sp["kl_share_max"], (name, "KL floor share", fig)
    if sp["target_kl"] is not None:
        fig["kl_stop_gap"] = min(o["margins"]["kl_stop"].min() for o in outs)
        assert fig["kl_stop_gap"] >= KL_STOP_MARGIN, (name, "KL stop", fig)
    if sp["recompute"]:
        fig["refreshes"] = [o["recomputed_epochs"] for o in outs]
        assert min(fig["refreshes"]) >= 1, (name, "a refresh in every cycle", fig)
        if sp["vtrace"] is not None:                                                 # every weight of every refresh away from both bars: the two fractions are exact counts
            fig["vtrace_gap"] = min(o["margins"]["vtrace"].min() for o in outs)
            fig["vtrace_fractions"] = [(o["vtrace_rho_clip_fraction"], o["vtrace_c_clip_fraction"]) for o in outs]
            assert fig["vtrace_gap"] >= RATIO_MARGIN, (name, "V-trace bars", fig)
            if name in ("H", "I"):                                                   # the bars do something and do not do everything
                assert all(0.1 <= f <= 0.9 for pair in fig["vtrace_fractions"] for f in pair), (name, "V-trace clip fractions", fig)
        if name in ("I", "I-batch"):                                                 # a truncated segment whose refreshed bootstrap is not the recorded one
            fig["final_moved"] = max(float(np.nanmax(o["refresh_moved"]["final"] / (ar.ABS + ar.REL * np.abs(o["refreshed_final_values"].astype(np.float64))))) for o in outs)
            assert fig["final_moved"] >= 100.0, (name, "refreshed final values", fig)
    if sp["demo"] is not None:
        fig["demo_redraws"] = [int(o["margins"]["demo_redraws"].sum()) for o in outs]
        fig["demo_coefs"] = [(o["demo_coef"], o["demo_coef_next"]) for o in outs]
        if name == "J":
            assert max(fig["demo_redraws"]) >= 1, (name, "a permutation redrawn inside an update", fig)
            assert outs[1]["demo_coef"] == outs[0]["demo_coef_next"] != outs[0]["demo_coef"], (name, "the coefficient's chain", fig)
    return fig


# ------------------------------------------------------------------------------------------------------------------------------------ the comparison
def compare(name, got, ref, twin=None, cycle=0, raw_adv_max=None, fp32_mode=None):
    """Every asserted quantity of ONE update: `got` (the device's result, the twin's or a mutant's) against the float64 `ref` -> [(quantity, distance, bound)]; a
    bound of 0 asks for equality.  Keys that `ref` does not hold are not expected in `got` either.
    twin: the fp32 twin's result of the same update, for the bounds that are stated relative to it (tests/test_c_c3_ppo_gpu.py's rule: no further from float64
    than 2 x the twin + 2e-4 of the scale); None: the floor alone.  fp32_mode: a bf16x3 case's {quantity: the fp32 mode's distance} (module docstring).
    The bounds are the project's (README, "Numerical tolerances"):
      losses        as rollout_gpu_common.check_losses; the KL scalars by kl_penalty_cases.kl_bound
      norms         2 fp32 ulps at the first step of the first cycle, where both sides hold the same parameters.  In a later cycle they differ by the
                    trajectory's error: the first step is judged like every other HERE, and the GPU test compares it at 2 ulps with a copy of the reference
                    set to the device's parameters
      diagnostics   1e-4 relative, counts exact; moments 1e-12 max|x| / 1e-9 relative
      finish        what the reward scale's 1e-9 propagates to: |dA| <= 1e-9 sum_l (gamma lam)^l |r| <= 1e-9 T clip for the raw advantages and the returns, and
                    2 x that over a segment's std for the normalised ones.  Their sums are formed in the kernels' order (wave_sum()), so without reward scaling
                    they are bitwise; the batch normalisation's sums run over segments' partials and are held to 1e-12 of the largest, as
                    tests/test_n_rollout_segments_gpu.py holds them."""
    sp = spec(name)
    rows = []
    add = lambda q, err, bound: rows.append((q, float(err), float(bound)))      # noqa: E731
    tw = lambda key, i: None if twin is None else twin[key][i]                    # noqa: E731
    x3 = sp["precision"] == "bf16x3"
    mode = {} if fp32_mode is None else fp32_mode                                 # bf16x3: {quantity: the fp32 mode's distance from ITS float64 reference}

    def traj(q, g, r, t, scale=None, tol=0.0):
        scale = abs(r) if scale is None else scale
        if x3:                                                                   # the fp32 mode in the twin's place, and what the gradient tolerance allows
            add(q, abs(g - r), TRAJ_FACTOR * mode.get(q, 0.0) + TRAJ_FLOOR * scale + tol)
        else:
            add(q, abs(g - r), TRAJ_FACTOR * (abs(t - r) if t is not None else 0.0) + TRAJ_FLOOR * scale)

    def stat(q, g, r, floor=0.0):
        bound = DIAG_REL * abs(r) + floor
        add(q, abs(g - r), max(bound, 4.0 * mode.get(q, 0.0)) if x3 else bound)
    for key in set(ref) | set(got):
        if key not in NOT_RETURNED:
            add("key " + key, 0.0 if (key in ref) == (key in got) else 1.0, 0.0)
    add("samples", abs(got["samples"] - ref["samples"]), 0)
    add("lengths", np.abs(np.asarray(got["lengths"]) - ref["lengths"]).max(), 0)
    add("steps", abs(len(got["losses"]) - len(ref["losses"])), 0)
    for i, (g, r) in enumerate(zip(got["losses"], ref["losses"])):
        add("loss[%d]" % i, abs(g["loss"] - r["loss"]), LOSS_REL * abs(r["loss"]) + 1e-4)
        add("value_loss[%d]" % i, abs(g["value_loss"] - r["value_loss"]), LOSS_REL * abs(r["value_loss"]))
        add("policy_loss[%d]" % i, abs(g["policy_loss"] - r["policy_loss"]), 1e-4)
        add("entropy_loss[%d]" % i, abs(g["entropy_loss"] - r["entropy_loss"]), LOSS_REL * abs(r["entropy_loss"]))
        add("prob_ratio[%d]" % i, abs(g["prob_ratio"] - r["prob_ratio"]), LOSS_REL * abs(r["prob_ratio"]))
        if "kl" in r:
            add("kl[%d]" % i, abs(g["kl"] - r["kl"]), r["kl_bound"])
            add("kl_penalty[%d]" % i, abs(g["kl_penalty"] - r["kl_penalty"]), ref["kl_coef"] * r["kl_bound"])
    if "grad_norms" in ref:
        for i, (g, r) in enumerate(zip(got["grad_norms"], ref["grad_norms"])):
            tol = ref["grad_norm_tols"][i] if x3 else 0.0                       # bf16x3: | |g'| - |g| | <= |g' - g| <= 1e-3 sqrt(sum_k n_k max_k^2)
            s_ref = ref["clip_scales"][i]
            s_tol = s_ref * tol / r if s_ref < 1.0 else 0.0
            if i == 0 and cycle == 0:                                           # the same parameters on both sides: the norm itself is compared
                add("grad_norm[0]", abs(g - r), tol if x3 else ULP2 * r)
                add("clip_scale[0]", abs(got["clip_scales"][0] - s_ref), s_tol if x3 else ULP2 * s_ref)
            else:
                traj("grad_norm[%d]" % i, g, r, tw("grad_norms", i), tol=tol)
                traj("clip_scale[%d]" % i, got["clip_scales"][i], s_ref, tw("clip_scales", i), tol=s_tol)
    if "minibatch_adv_stats" in ref:
        gs, rs_ = np.asarray(got["minibatch_adv_stats"]), ref["minibatch_adv_stats"]
        add("minibatch steps", abs(len(gs) - len(rs_)), 0)
        if len(gs) == len(rs_):
            a_max = raw_adv_max if raw_adv_max is not None else float(np.nanmax(np.abs(ref["raw_advantages"])))
            add("minibatch count", np.abs(gs[:, 0] - rs_[:, 0]).max(), 0)
            base = MOMENT_MEAN * a_max + 1e-9 * sp["T"] * REWARD_CLIP
            if "minibatch_stat_tols" in ref and ref["minibatch_stat_tols"].any():   # behind a refresh: what its raw advantages' bounds allow the mean and the std (normalised_bound)
                tols = ref["minibatch_stat_tols"]
                add("minibatch mean", (np.abs(gs[:, 1] - rs_[:, 1]) / (base + tols[:, 0])).max(), 1.0)
                add("minibatch std", (np.abs(gs[:, 2] - rs_[:, 2]) / (base + tols[:, 1])).max(), 1.0)
                if twin is not None and not x3 and len(twin["minibatch_adv_stats"]) == len(rs_):      # (TWIN_HELD's rule: this bound too is > 100 x the twin's distance in every case)
                    behind = tols[:, 1] > 0
                    add("minibatch std (4 x the twin)", np.abs(gs[behind, 2] - rs_[behind, 2]).max(), 4.0 * np.abs(twin["minibatch_adv_stats"][behind, 2] - rs_[behind, 2]).max())
            else:
                add("minibatch mean", np.abs(gs[:, 1] - rs_[:, 1]).max(), base)
                add("minibatch std", np.abs(gs[:, 2] - rs_[:, 2]).max(), base)
    if "epochs" in ref:
        add("epochs_run", abs(got["epochs_run"] - ref["epochs_run"]), 0)
        add("stopped_early", float(got["stopped_early"] != ref["stopped_early"]), 0)
        for i, (g, r) in enumerate(zip(got["epochs"], ref["epochs"])):
            for k, v in r.items():
                if k in ("samples", "clip_fraction", "value_clip_fraction", "value_grad_zero_fraction", "clipped_steps"):
                    add("%s[%d]" % (k, i), abs(g[k] - v), 0)
                elif k == "grad_norm_max":
                    traj("%s[%d]" % (k, i), g[k], v, None if twin is None or i >= len(twin["epochs"]) else twin["epochs"][i][k],
                         tol=float(ref["grad_norm_tols"].max()) if x3 else 0.0)
                else:                                                                # k1 is a mean of differences of two fp32 log-probabilities and may cancel: K1_FLOOR
                    stat("%s[%d]" % (k, i), g[k], v, K1_FLOOR * ref["logp_old_max"] if k == "approx_kl_k1" else 0.0)
    if "kl" in ref:
        for k in ("kl", "kl_std", "kl_mean_part"):
            stat("kl." + k, got["kl"][k], ref["kl"][k])
        add("kl.samples", abs(got["kl"]["samples"] - ref["kl"]["samples"]), 0)
        add("kl_coef", abs(got["kl_coef"] - ref["kl_coef"]), 0)
        add("kl_coef_next", abs(got["kl_coef_next"] - ref["kl_coef_next"]), 0)
    prop = 1e-9 * sp["T"] * REWARD_CLIP if "return_rms" in ref else 0.0
    if "return_rms" in ref:
        rec = ~np.isnan(ref["discounted_returns"])
        g_max = float(np.abs(ref["discounted_returns"][rec]).max())
        add("return_rms.count", abs(got["return_rms"]["count"] - ref["return_rms"]["count"]), 0)
        add("return_rms.mean", abs(got["return_rms"]["mean"] - ref["return_rms"]["mean"]), MOMENT_MEAN * g_max)
        add("return_rms.var", abs(got["return_rms"]["var"] - ref["return_rms"]["var"]), MOMENT_VAR * ref["return_rms"]["var"])
        add("reward_scale_den", abs(got["reward_scale_den"] - ref["reward_scale_den"]), MOMENT_VAR * ref["reward_scale_den"])
        add("discounted_returns", float(not np.array_equal(got["discounted_returns"], ref["discounted_returns"], equal_nan=True)), 0)
        add("return_carry", float(not np.array_equal(got["return_carry"], ref["return_carry"])), 0)
        add("scaled_rewards NaN", float(not np.array_equal(np.isnan(got["scaled_rewards"]), ~rec)), 0)
        sr = ref["scaled_rewards"][rec]
        add("scaled_rewards", (np.abs(got["scaled_rewards"][rec] - sr) - np.spacing(np.abs(sr)) - MOMENT_VAR * np.abs(sr)).max(), 0)
        add("reward_clip_fraction", abs(got["reward_clip_fraction"] - ref["reward_clip_fraction"]), 0)
    rec = ~np.isnan(ref["raw_advantages"])
    for k in ("raw_advantages", "returns", "advantages"):
        add(k + " NaN", float(not np.array_equal(np.isnan(got[k]), ~rec)), 0)
    add("raw_advantages", np.abs(got["raw_advantages"][rec] - ref["raw_advantages"][rec]).max(), prop)
    add("returns", np.abs(got["returns"][rec] - ref["returns"][rec]).max(), prop)
    stds = []                                                                        # the smallest std a normalisation divided by
    if sp["kind"] == "continuous" and sp["normalize"] == "batch":
        stds = [ref["raw_advantages"][rec].std()]
    else:
        stds = [ref["raw_advantages"][e, first:first + n].std() for e, first, n in ref["segment_list"] if n > 1]
    batch_sums = 1e-12 * float(np.abs(ref["advantages"][rec]).max()) if sp["normalize"] == "batch" else 0.0
    add("advantages", np.abs(got["advantages"][rec] - ref["advantages"][rec]).max(), (2 * prop / min(stds) if prop else 0.0) + batch_sums)
    def per_entry(q, g, r, b):
        """max |g - r| / b over the entries `r` holds, NaN in the same places; an entry whose bound is 0 asks for equality."""
        g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
        if g.shape != r.shape or not np.array_equal(np.isnan(g), np.isnan(r)):
            return add(q, float("inf"), 1.0)
        ok = ~np.isnan(r)
        d, b = np.abs(g - r)[ok], np.broadcast_to(b, r.shape)[ok]
        with np.errstate(divide="ignore", invalid="ignore"):
            add(q, np.where(b > 0, d / b, np.where(d > 0, np.inf, 0.0)).max() if ok.any() else 0.0, 1.0)
    # ---- advantage recomputation and V-trace: the last refresh's tables.  Values by the project's value bound (advantage_recomputation_cases.distance), weights by
    # the log pi bound on both log-probabilities, the finish's outputs by its own recurrence run on those per-entry bounds (Trainer.finish_bounds): no constant of
    # their own.  The fp64 triple is compared (no fp32 table: no ulp is added)
    if "recomputed_epochs" in ref:
        add("recomputed_epochs", abs(got.get("recomputed_epochs", -1) - ref["recomputed_epochs"]), 0)
    if "refreshed_values" in ref and "refreshed_values" in got:
        add("refreshed_values", ar.distance(got["refreshed_values"], ref["refreshed_values"]), 1.0)
        if "refreshed_final_values" in ref:
            add("refreshed_final_values", ar.distance(got["refreshed_final_values"], ref["refreshed_final_values"]), 1.0)
        rb = ref["refresh_bounds"]
        if "refreshed_importance_weights" in ref:
            per_entry("refreshed_importance_weights", got["refreshed_importance_weights"], ref["refreshed_importance_weights"], rb["b_weights"])
            add("vtrace_rho_clip_fraction", abs(got["vtrace_rho_clip_fraction"] - ref["vtrace_rho_clip_fraction"]), 0)
            add("vtrace_c_clip_fraction", abs(got["vtrace_c_clip_fraction"] - ref["vtrace_c_clip_fraction"]), 0)
        per_entry("refreshed_raw_advantages", got["refreshed_raw_advantages"], ref["refreshed_raw_advantages"], rb["b_raw"])
        per_entry("refreshed_returns", got["refreshed_returns"], ref["refreshed_returns"], rb["b_ret"])
        per_entry("refreshed_advantages", got["refreshed_advantages"], ref["refreshed_advantages"], rb["b_adv"] + batch_sums)
        # the derived bounds of TWIN_HELD are looser than 100 x the fp32 twin's own distance in every case (profiles/r41_rollout_newer_settings.md): those
        # quantities are also held to 4 x the twin's distance on the same tables (fp32 mode; in bf16x3 the README's bound for the mode is the derived one alone)
        for key in TWIN_HELD:
            if twin is not None and not x3 and key in ref and key in twin and np.array_equal(np.isnan(got[key]), np.isnan(ref[key])):
                ok = ~np.isnan(ref[key])
                add(key + " (4 x the twin)", np.abs(got[key] - ref[key])[ok].max(), 4.0 * np.abs(twin[key] - ref[key])[ok].max())
    # ---- the demonstration term: the rows exactly (the setting's own stream), demo_loss 1e-4 of its absolute terms (tests/demo_term_cases.py's row), the rest relative
    if "demo_losses" in ref:
        add("demo steps", abs(len(got["demo_losses"]) - len(ref["demo_losses"])) + abs(len(got["demo_rows"]) - len(ref["demo_rows"])), 0)
        add("demo_rows", float(not all(np.array_equal(g, r) for g, r in zip(got["demo_rows"], ref["demo_rows"]))), 0)
        add("demo_coef", abs(got["demo_coef"] - ref["demo_coef"]), 0)
        add("demo_coef_next", abs(got["demo_coef_next"] - ref["demo_coef_next"]), 0)
        for i, (g, r) in enumerate(zip(got["demo_losses"], ref["demo_losses"])):
            add("demo_loss[%d]" % i, abs(g["demo_loss"] - r["demo_loss"]), LOSS_REL * r["abs_terms"])
            add("demo_mean_sq_error[%d]" % i, abs(g["mean_sq_error"] - r["mean_sq_error"]), LOSS_REL * abs(r["mean_sq_error"]))
    if "observation_rms" in ref:
        x_max = float(np.nanmax(np.abs(ref["raw_states"])))
        add("observation_rms.count", abs(got["observation_rms"]["count"] - ref["observation_rms"]["count"]), 0)
        add("observation_rms.mean", np.abs(got["observation_rms"]["mean"] - ref["observation_rms"]["mean"]).max(), MOMENT_MEAN * x_max)
        add("observation_rms.var", (np.abs(got["observation_rms"]["var"] - ref["observation_rms"]["var"]) - MOMENT_VAR * ref["observation_rms"]["var"]).max(), 0)
        add("observation_clip_fraction", np.abs(got["observation_clip_fraction"] - ref["observation_clip_fraction"]).max(), 0)
    if "raw_states" in got:
        ok = ~np.isnan(ref["raw_states"]).any(-1)
        add("raw_states", float(not np.array_equal(np.asarray(got["raw_states"], np.float32)[ok].view(np.int32), ref["raw_states"][ok].view(np.int32))), 0)
        d_states = np.abs(np.asarray(got["states"], np.float64)[ok] - np.asarray(ref["states"], np.float64)[ok])
        add("states", (d_states - ref["state_bound"][ok]).max(), 0)                   # the bootstrap slots too
    if "params" in got:
        for k, e_d, e_t, scale in trajectory_errors(got["params"], ref["params"] if twin is None else twin["params"], ref["params"], ref["p0"]):
            if x3:
                add("params " + k, e_d, TRAJ_FACTOR * mode.get("params " + k, 0.0) + TRAJ_FLOOR * scale)
            else:
                add("params " + k, e_d, TRAJ_FACTOR * e_t + TRAJ_FLOOR * scale)
    return rows


def worst(rows):
    """-> (the largest distance / bound, its row); an exceeded bound of 0 counts as infinity."""
    best = (-1.0, None)
    for q, err, bound in rows:
        ratio = (float("inf") if err > 0 else 0.0) if bound <= 0 else err / bound
        if not ratio <= best[0]:
            best = (ratio, (q, err, bound))
    return best
