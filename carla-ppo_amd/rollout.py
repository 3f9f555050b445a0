"""One environment step of the rollout loop as ONE device call.

The reference does, per simulator step (vae_common.py:45-61, train.py:142, run_eval.py:54):

    frame = env.observation.astype(np.float32) / 255.0
    state = np.append(vae.encode([frame])[0], [steer, throttle, speed])          # sess.run #1, host round trip
    action, value = model.predict(state, write_to_summary=True)                  # sess.run #2, host round trip

RolloutStep does the same arithmetic in one C-ABI call (mi_rollout_step: raw uint8 frame -> /255 -> conv x 4 -> mean -> [z, measurements] ->
policy / value heads; exact fp32 on the master weights; eight launches).  By default nothing is copied: the frame bytes, the measurements and
the exploration noise sit in one pinned host buffer the first kernel reads over PCIe (38 KB), and the last kernel stores (action, value, z)
into pinned host memory; io="device" stages both through HBM with one copy each way (5 us slower on the measured box).
No CPU fallback: needs the HIP library and a GPU.

    step = RolloutStep(vae, ppo)
    action, value, state = step(env.observation, [steer, throttle, speed])       # state: float64 [z_dim + k], as np.append returns it

The split-K layers accumulate with fp32 atomics, so two calls on the same frame can differ in the last bit (1e-7 relative).

BatchedRolloutStep is the same step for n environments per call (mi_rollout_step_batch: the same eight launches, the rows of every layer running over the
environments; the flat layers' MFMA rows, 31 of 32 empty at one frame, carry the environments):

    step = BatchedRolloutStep(vae, ppo, num_envs=8)
    actions, values, states = step(frames_u8, measurements)                      # [n, H, W, 3] uint8, [n, k] -> [n, A], [n], float64 [n, z_dim + k]

On the measured box one call takes 70 / 96 / 310 us for 2 / 8 / 64 environments against 127 / 504 / 3840 us for a loop of RolloutStep calls; at one environment it
is 3 us slower than RolloutStep (66 against 63 us).  The two-call path (vae.encode + ppo.predict of the batch) was not faster at any measured E up to 64 (3.0 x
slower at E = 1, 1.3 x at E = 64; profiles/r08_rollout_batch.md).

RolloutBuffer joins that step to the PPO update without a trip through the host: its step is the batched step with RECORDING heads (mi_rollout_step_batch_rec), which leave
the state [z | measurements], the action and the value of every environment in device tables of num_envs x (horizon + 1) rows -- the tables mi_ppo_train_step_idx gathers
from.  A row is one episode segment, as the reference's loop collects it (train.py:139-207): it ends when its environment reports done or reaches the horizon, and the slot
behind its last step holds the bootstrap state and value (train.py:172).  update() finishes the ragged rows in one launch (mi_rollout_finish: GAE, returns, per-row
normalisation, fp64, bit for bit the dense kernels on each row alone) and runs the epochs of shuffled minibatches from the tables:

    buf = RolloutBuffer(vae, ppo, num_envs=8, horizon=128)
    buf.reset()
    live = np.arange(8)
    while len(live):
        actions, values, states = buf.step(frames[live], measurements[live], env_ids=live)
        rewards, dones = simulator(actions)                                     # host arrays, 16 bytes per step
        buf.outcome(rewards, dones, env_ids=live)
        live = live[(~dones) & (buf.lengths[live] < buf.horizon)]
    buf.bootstrap(last_frames, last_measurements)                               # every environment that was stepped: closes the rows
    out = buf.update(gamma=0.99, lam=0.95, num_epochs=3, batch_size=32)

ContinuousRolloutBuffer is that buffer for vectorised collection: every environment steps `horizon` times per update, and a simulator that reports done hands back its
reset observation and goes on.  A lane (the horizon + 1 table rows of an environment) then holds several episode SEGMENTS; update() finishes them in one call
(mi_rollout_finish_segments: GAE, returns and normalisation per segment, each bit for bit the dense kernels on that segment alone; a segment that ends in a done bootstraps
from 0.0 and never reads the slot behind it, which holds the next episode's first value) and otherwise does what RolloutBuffer.update does.  normalize="batch" normalises the
advantages over all samples of the update instead (tail segments of one or two steps otherwise come out as 0 or +-1):

    buf = ContinuousRolloutBuffer(vae, ppo, num_envs=8, horizon=128)
    buf.reset()
    for _ in range(buf.horizon):                                   # every call carries all 8 environments
        actions, values, states = buf.step(frames, measurements)
        rewards, dones, frames, measurements = simulators_step(actions)   # a simulator that reports done returns its reset observation
        buf.outcome(rewards, dones)
    need = buf.rows.needs_bootstrap()
    buf.bootstrap(frames[need], measurements[need], env_ids=need)
    out = buf.update(num_epochs=3, batch_size=32)                  # exactly 8 x 128 samples

An episode can also stop WITHOUT being terminal and be followed by a reset in the same lane: a simulator-side step or time limit, a simulator that timed out and was
restarted, a route switch.  Reported as a done it pulls the value target of its last steps towards "the car crashed here"; not reported at all, GAE runs across the reset.
truncate() is the third way for a segment to end: it takes the FINAL observation of the stopped episodes -- no step of the lane, the lane's next step is the reset
observation -- and one value-only device call (mi_rollout_value_batch_rec: encoder chain, value trunk, value head) leaves its value in `buf.final_values` at the table row
of the episode's last step; update() then bootstraps that segment from it (mi_rollout_finish_segments_boot) and never reads the slot behind it:

    for _ in range(buf.horizon):
        actions, values, states = buf.step(frames, measurements)
        rewards, dones, truncated, frames, measurements, final_frames, final_measurements = simulators_step(actions)   # done or truncated: frames[e] is the reset observation
        buf.outcome(rewards, dones)                                # a truncated step reports done False
        cut = np.nonzero(truncated & ~dones)[0]
        if len(cut):
            buf.truncate(final_frames[cut], final_measurements[cut], env_ids=cut)   # after outcome(), before these lanes' next step
    need = buf.rows.needs_bootstrap()                              # a lane whose last step is a done or truncated needs none
    buf.bootstrap(frames[need], measurements[need], env_ids=need)
    out = buf.update(num_epochs=3, batch_size=32)                  # out["segment_truncated"], out["final_values"]

A collection on which truncate() is never called takes the path it always took (mi_rollout_finish_segments, the same launches).

Both buffers can watch how far an update moves the policy.  update_with_diagnostics() is update() plus one forward-only statistics pass over all valid rows after
every epoch (mi_ppo_update_stats_idx: the current policy against the cached log pi_old; ordered double-precision sums, bitwise reproducible), and target_kl ends the
epochs once the approximate KL to the old policy (k3, mean of r - 1 - log r) is greater than it:

    out = buf.update_with_diagnostics(num_epochs=10, batch_size=32, target_kl=0.03)
    for e in out["epochs"]:                                        # one dict per epoch that ran
        print(e["approx_kl"], e["clip_fraction"], e["explained_variance"])
    out["epochs_run"], out["stopped_early"]                        # e.g. 4, True

update() itself is unchanged: the same launches, the same numpy RNG draws, the same keys.

Both buffers report the size of every SGD step once the policy clips its gradient by the global L2 norm (PPO.set_max_grad_norm, or MI355_PPO_MAX_GRAD_NORM under
the unchanged reference scripts; tf.clip_by_global_norm in front of Adam: an ordered double-precision sum of squares over the 13 policy/ variables, no atomics,
bitwise reproducible):

    ppo.set_max_grad_norm(0.5)                                     # float("inf"): measure the norm, never clip;  None: off
    out = buf.update(num_epochs=10, batch_size=32)
    out["grad_norms"], out["clip_scales"]                          # float32 [number of SGD steps]: the norm before clipping, the factor applied (1.0 = not clipped)

and every dict in `epochs` of update_with_diagnostics() gains `grad_norm_max` and `clipped_steps`.  With the setting off none of these keys appears, and the update
makes the launches it always made.

A policy of more than 96 inputs -- a VAE of more than 93 latents: train_vae.py --z_dim 128, ConvVAE's default of 512 -- is outside the fused kernels' default range:
update() then gathers every minibatch on the host side and evaluates the old policy in every step, and update_with_diagnostics(), PPO.set_value_clip() and
PPO.set_kl_penalty() raise ValueError.  ppo.set_wide_inputs() (MI355_PPO_WIDE_INPUTS=1 under the unchanged reference scripts) extends the range to 1024 inputs:
the step classes, both buffers and every setting below then take the routes they take for the shipped 67-input agent.  State tables stay below 2 GiB.

Both buffers can clip the value loss as the original PPO2 code does (baselines ppo2; clip_vloss / clip_range_vf elsewhere).  The tables already hold the value of
every step as it was when the data was collected; with PPO.set_value_clip(eps_v) every SGD step of update() passes that table along (mi_ppo_train_step_vclip: one more
gather per sample in the loss kernel) and a sample's value term becomes max((V - R)^2, (V_c - R)^2) with V_c = V clamped into V_old +- eps_v: the value net gets no
gradient from a sample whose value has already moved further than eps_v from V_old towards its return.  `value_loss` in the loss records is then the clipped objective:

    ppo.set_value_clip(0.2)                                        # float("inf"): the clipped step, never a clipped sample;  None: off
    out = buf.update_with_diagnostics(num_epochs=10, batch_size=32)
    for e in out["epochs"]:
        print(e["value_clip_fraction"], e["value_loss_clipped"], e["value_grad_zero_fraction"])

The three keys come from one more small launch pair per statistics chunk (mi_ppo_value_clip_stats over the value table the statistics pass writes; ordered double sums,
no atomics) and are read back with the epoch's other sums.  There is no environment knob (the reference's train.py passes no old values), PPO.train() refuses to run
with the setting on, and the policy must be on the fused kernels (ValueError otherwise, before anything is launched).  With the setting off the keys, launches and numbers
are what they were.

Both buffers honour dual-clip PPO (Ye et al. 2020; PPO.set_dual_clip(c), or MI355_PPO_DUAL_CLIP under the unchanged reference scripts).  Many epochs per collection,
refreshed advantages and demonstration rows let the ratio r stray from 1, and the clipped surrogate of a sample with A < 0 and r > 1 + eps is r A, which grows with r
without bound; with a constant c > 1 that sample's term becomes the constant c A once r has passed c, and it gives the policy no gradient.  The setting lives on
the engine, so update() needs nothing new; update_with_diagnostics() also reports what it did:

    ppo.set_dual_clip(3.0)                                         # float("inf"): the setting on, never a dual-clipped sample;  None: off
    ppo.set_loss_coefficients(epsilon=0.1, entropy_scale=0.005)    # a clip-range / entropy schedule on the live engine: Adam state and tables stay
    out = buf.update_with_diagnostics(num_epochs=10, batch_size=32)
    for e in out["epochs"]:
        print(e["dual_clip_fraction"], e["negative_advantage_fraction"], e["surrogate_mean"], e["surrogate_mean_unclipped"])

The four keys come from one more small launch pair per statistics chunk (mi_ppo_dual_clip_stats over the log pi_theta table the statistics pass writes, the cached
log pi_old and the advantage table the epoch's steps gathered from -- the minibatch table with per-minibatch normalisation; ordered double sums, no atomics) and are
read back with the epoch's other sums.  The policy must be on the fused kernels (ValueError otherwise, before anything is launched).  With the setting off the keys,
launches and numbers are what they were.

Both buffers can scale the rewards by the running standard deviation of the discounted return, as every code base does that eps_v = 0.2 and max_grad_norm = 0.5 come
from (baselines VecNormalize and its descendants).  eps_v, value_scale and the gradient norm are in units of the return, and CARLA's reward functions differ by orders of
magnitude; the advantages are normalised already, the rewards -- and with them the returns, the value targets and the value net's gradients -- are not.  With
set_reward_scaling() one device call of its own (mi_rollout_scale_rewards: four small launches, fp64, ordered sums, no atomics, bitwise reproducible) runs between the
upload of the rewards and the finish call: it continues every lane's discounted return G = G * gamma + r from the carry the last update left (0.0 behind a done or a
truncated step), merges the moments of the collection's G into the running {count, mean, M2} kept on the device (Chan / Welford), and hands the finish kernels
r / sqrt(var + epsilon), clamped into +-clip.  The finish kernels, the SGD steps and the statistics pass are the code they were:

    buf.set_reward_scaling(clip=10.0, epsilon=1e-8)               # frozen=True: scale by the statistics as they are (evaluation, fine-tuning);  None: off
    out = buf.update(num_epochs=10, batch_size=32)
    out["return_rms"], out["reward_scale_den"]                     # {"count", "mean", "var"} of the discounted returns so far, the divisor of this update
    out["scaled_rewards"], out["discounted_returns"]               # fp64 [num_envs, T], NaN beyond a lane's length
    out["reward_clip_fraction"], out["return_carry"]               # the share of rewards the clamp changed to +-clip; fp64 [num_envs]
    ckpt = buf.reward_scaling_state()                              # ... buf.load_reward_scaling_state(ckpt) in the run that resumes
    buf.zero_return_carry([3])                                     # environment 3 was reset without a done or a truncation being reported

Two deviations from baselines, both on purpose: a collection is scaled by ONE factor, from statistics that already include it ("update ret_rms, then divide" per update
instead of per step -- per-step scaling needs the reward on the device at every step and puts the rewards of one collection on different scales), and the statistics
start from count 0 instead of the prior count = 1e-4, var = 1.  reset() starts a collection and touches neither the statistics nor the carries.  A non-finite reward in
a recorded step would poison the statistics for good: update() raises ValueError before anything is launched or changed.  The value error and the explained variance of
update_with_diagnostics() are then measured on the scaled returns.  With the setting off none of these keys appears and the update makes the launches it always made.

Both buffers can normalise the advantages PER MINIBATCH, inside the SGD loop, as the libraries do whose defaults clip_range, max_grad_norm = 0.5 and target_kl come from
(SB3 normalize_advantage=True, CleanRL norm_adv=True): the scale of every step's policy gradient is then set by that step's batch_size samples, not by a segment
(normalize="segment", train.py:176-177) or by the whole collection (normalize="batch").  The finish call runs as it always did; with set_minibatch_normalization() one
device call per epoch (mi_ppo_minibatch_advantages: one launch, one block per minibatch, fp64, ordered sums, no atomics, bitwise reproducible) runs between the upload
of the epoch's shuffled rows and its first step: it takes the RAW advantages the finish call left, normalises every minibatch of the epoch by its own mean and std
((a - mean) / (std + 1e-8)) and writes a second fp32 table, which the epoch's SGD steps gather from in place of `advantages`.  The steps themselves are the code they were:

    buf.set_minibatch_normalization()                              # ddof=0: population std;  ddof=1: torch's .std(), what SB3 / CleanRL divide by;  None: off
    out = buf.update(num_epochs=10, batch_size=32)
    out["minibatch_adv_stats"]                                     # float64 [number of SGD steps, 3]: {count, mean, std} of every step's raw advantages
    out["minibatch_advantages"]                                    # float32 [num_envs, T]: what the last epoch's steps read;  out["advantages"]: the finish call's, NOT read by the steps

Two deviations from SB3, both on purpose: ddof=0 by default (the population std, as everywhere else in this project; SB3 and CleanRL use the sample std: pass ddof=1
to compare), and a one-sample minibatch -- the partial last one of an epoch -- yields 0 (its std is 0 with either ddof) instead of being left unnormalised: that step's
surrogate term has no gradient, its value and entropy terms have theirs.  The numpy RNG draws, the launches of every step, the statistics pass of update_with_diagnostics() and reward scaling are
unchanged; `stage_times` gains "minibatch_norm", which is also part of "sgd".  With the setting off none of these keys appears and the update makes the launches it
always made.

Both buffers can normalise the OBSERVATIONS by their running mean and standard deviation -- the other half of VecNormalize.  The policy's input is [z | steer, throttle,
speed]: a speed of 0..30 next to 66 columns of unit scale, in front of settings (max_grad_norm = 0.5, eps_v = 0.2, the learning rate) that were tuned for standardised
inputs.  The state is assembled inside the step's device call, so the normalisation lives there too: with set_observation_normalization() step(), bootstrap() and
truncate() go through mi_rollout_step_batch_norm / mi_rollout_value_batch_norm -- one more launch (rollout_obs_norm_kernel) between the mean layer and trunk layer 1
writes clamp((s - mean32[j]) * inv32[j], -clip, +clip) per column (fp32: one subtract, one multiply; clip = inf is allowed) into a buffer trunk layer 1 then reads.  The
table `states` holds the NORMALISED rows, so log pi_old, the SGD steps, the statistics pass and every other reader of that table are the code they were and see the inputs
the policy acted on; a second fp32 table `raw_states` takes the raw rows through the existing recording heads.  The last launch of update() (mi_rollout_obs_stats: fp64,
ordered sums, no atomics, bitwise reproducible) merges the raw rows of rows.valid_rows() -- recorded steps only, no bootstrap slot -- into {count, mean[din], M2[din]} on
the device (Chan / Welford per column) and derives mean32 = float32(mean), inv32 = float32(1 / sqrt(M2 / count + epsilon)) for the next collection:

    buf.set_observation_normalization(clip=10.0, epsilon=1e-8)     # frozen=True: use the statistics, never update them;  normalize_latents=False;  None: off
    buf.reset(); ...warm-up steps...; buf.merge_observation_statistics(); buf.reset()      # optional: the first collection otherwise clamps a raw speed of 30 to clip
    out = buf.update(num_epochs=10, batch_size=32)
    out["observation_rms"]                                         # {"count", "mean" [din], "var" [din]} after this update's merge
    out["observation_clip_fraction"]                               # float64 [din]: the share of this collection's entries the clamp put at +-clip
    ckpt = buf.observation_normalization_state()                   # ... buf.load_observation_normalization_state(ckpt) in the run that resumes
    step = BatchedRolloutStep(vae, ppo, num_envs=1); step.set_observation_normalization(ckpt)      # evaluation: applies the statistics, never updates them
    ppo.predict(normalize_observations(states, ckpt))              # the same formula in numpy float32, for callers that feed host states

Two deviations from VecNormalize, both on purpose and the ones reward scaling made: ONE set of statistics per collection (VecNormalize updates obs_rms at every step,
before it normalises that step; here nothing changes mean32 / inv32 between two updates, so every row of a collection is normalised alike and an update trains on the
inputs the policy acted on), and the statistics start from count 0 (mean 0, inv_std exactly 1.0: the first collection is the identity apart from the clamp) instead of the
prior count = 1e-4.  normalize_latents=False writes mean 0 / inv_std 1 for the first z_dim columns (their moments are still tracked, the clamp still applies): for VAEs
whose latents are at prior scale already, and for latent columns of near-zero variance, which would otherwise be blown up to +-clip.  The states a step RETURNS, and the
latents in its output row, stay the raw observation.  An update that raises leaves the statistics as they were; a recorded observation that is not finite (NaN,
+-inf) is such a case -- the merge kernels refuse the whole batch, since one NaN would stay in mean / M2 for good, and update() / merge_observation_statistics() raise
ValueError behind that launch (the SGD steps of that update have run by then; the statistics are as they were); reset() does not touch them; RolloutStep, the
single-frame entry, has no normalised form (ValueError: use BatchedRolloutStep(num_envs=1)).  `stage_times` gains "observation_stats".  With the setting off none of
these keys appears, no table is allocated and every call makes the launches it always made.

Adaptive KL penalty (the PPO paper's other objective, section 4; no setter here: the buffers read ppo.kl_penalty / ppo.kl_target as they read ppo.value_clip):

    ppo.set_kl_penalty(0.2, target=0.01)                           # beta x mean KL(pi_old || pi_theta) added to the clipped surrogate; target None: beta stays fixed
    out = buf.update(num_epochs=3, batch_size=32)
    out["kl"], out["kl_coef"], out["kl_coef_next"], out["kl_adapted"]

With it on, the pass that caches log pi_old also fills `mean_old` [n_table_rows, A] (mi_ppo_old_policy_cache), every SGD step goes through mi_ppo_train_step_kl
(together with the recorded values when value clipping is on as well) and its record in `losses` gains `kl` / `kl_penalty`; behind the last epoch one forward-only pass
(mi_ppo_kl_stats_idx over valid_rows() in chunks of 4096, one readback; `stage_times` gains "kl_stats") measures the exact KL under the parameters the update ended
with -- `kl` = {"samples", "kl", "kl_std", "kl_mean_part"} -- and PPO.adapt_kl_penalty applies the paper's rule on the host: kl < target / 1.5 halves beta, kl >
1.5 target doubles it, both strict.  `kl_coef` is the beta this update used, `kl_coef_next` the one the next will; `kl_adapted` is False when there is no target or the
measured KL is not finite (beta then stays, nothing is raised).  All of it comes before the observation-statistics launch.  beta and the target are not part of
ppo.state_dict(): ppo.kl_penalty_state() / load_kl_penalty_state() carry them.  With the setting off none of these keys appears, no table is allocated and not one
launch or readback is added.

The encoder may be an MlpVAE (the reference's --vae_model_type mlp).  BatchedRolloutStep, RolloutBuffer and ContinuousRolloutBuffer then go through
mi_mlp_rollout_step_batch / mi_mlp_rollout_value_batch (an MlpVaeDevice says rollout_kind = "mlp"; its handle never reaches the mi_rollout_* entries, which read theirs
as a ConvVAE engine): a clear launch, layer 1 of the encoder straight from the camera bytes (csrc/rollout_mlp.hip: the fp32 master kernel streamed once per call, every
frame byte fetched once, K split over the chip and met by fp32 atomics), the remaining hidden layers and the mean head as flat split-K layers, then the trunks, heads,
normaliser and value-only heads of the ConvVAE step -- exact fp32 on the master weights whatever the VAE's storage type.  Everything above works unchanged: recording,
truncation, diagnostics, value clipping, the KL penalty, reward scaling, observation and minibatch normalisation.  The scratch is 4 n (sum of the encoder widths +
z_dim) bytes (mi_mlp_rollout_workspace_bytes).  On the measured box one call takes 84 / 91 / 223 us for 1 / 8 / 64 environments against 185 / 213 / 389 us for the
two-call path on the same model (profiles/r27_mlp_rollout.md).  RolloutStep, the single-frame entry, has no MLP form (ValueError: use BatchedRolloutStep(vae, ppo,
num_envs=1)).

The step classes and both buffers can STACK LATENTS.  One frame per step tells a feed-forward policy nothing about how fast another car is closing, the yaw rate, or a
light that has just changed; the usual remedy is to stack the last k observations, and here the observation is compressed already, so the cheap form is
s_t = [z_t | z_{t-1} | .. | z_{t-k+1} | measurements_t] with input_dim = k z_dim + n_meas.  Built by the classmethod `stacked(.., latent_stack=k)` of its class (the constructor's arguments and k = 2 .. 16, at most 1024 inputs) the step owns a
device-resident `history` [num_envs, k - 1, z_dim] (fp32, zeros; slot 0 is the latent of the lane's previous step) and a host bool per lane, "fresh".  Every call is then
mi_rollout_step_batch_stack / mi_rollout_value_batch_stack (mi_mlp_.. with an MlpVAE) -- one more launch, rollout_stack_kernel, where the normaliser runs: a block per row
assembles the state from the frame's latent and its lane's history (a fresh lane repeats its own latent k times, as frame stacking pads with the first observation),
stores it for trunk layer 1 and into the tables, normalises it where observation normalisation is on, hands the older latents back next to `out`, and behind a barrier
shifts the lane's history.  The lanes and their fresh flags travel behind the table rows in the pinned input buffer; the states a call returns are float64
[n, k z_dim + n_meas], bitwise the raw row the kernel assembled:

    ppo = PPO(np.array([4 * 64 + 3]), space, ...); ppo.set_wide_inputs()       # a policy of more than 96 inputs wants ppo.set_wide_inputs() for its update
    buf = ContinuousRolloutBuffer.stacked(vae, ppo, num_envs=8, horizon=128, latent_stack=4)
    buf.reset()
    for _ in range(buf.horizon):
        actions, values, states = buf.step(frames, measurements)            # advances the history of the stepped lanes
        rewards, dones, truncated, frames, measurements, final_frames, final_measurements = simulators_step(actions)
        buf.outcome(rewards, dones)                                         # done: that lane's next step is fresh
        cut = np.nonzero(truncated & ~dones)[0]
        if len(cut):
            buf.truncate(final_frames[cut], final_measurements[cut], env_ids=cut)   # valued on the episode's history, then fresh
    need = buf.rows.needs_bootstrap()
    buf.bootstrap(frames[need], measurements[need], env_ids=need)           # reads the history and does NOT advance it: the next collection steps this observation again
    out = buf.update(num_epochs=3, batch_size=32)
    buf.reset()                                                             # touches neither the history nor the flags: an episode may continue across an update
    buf.restart_history([3])                                                # environment 3 was reset without a done or a truncation being reported
    ckpt = buf.history_state()                                              # ... buf.load_history_state(ckpt) in the run that resumes
    step = BatchedRolloutStep.stacked(vae, ppo, num_envs=1, latent_stack=4) # evaluation: step.step(frames, measurements, env_ids=..), step.restart() at an episode's start

The tables `states` / `raw_states` are input_dim wide as they always were, and update(), update_with_diagnostics() and every setting above are the code they were.  The
"latent columns" of observation normalisation (normalize_latents=False, the z_dim kept in its state) are the first k z_dim columns.  RolloutStep, the single-frame
entry, has no stacked form (RolloutStep.stacked raises ValueError: use BatchedRolloutStep.stacked(num_envs=1)).  At k = 4 and 64 latents the recording call was measured at +6 to +7 / +8 to +10 / +18 to +21 us for 1 / 8 / 64 environments
(one more launch, a trunk layer 1 of 259 inputs instead of 67, the older latents written out; profiles/r29_latent_stack.md).  With the setting off no tensor
is allocated and every call makes the launches it always made.

Single rank only (ragged rows give ranks different numbers of gradient all-reduces).

DemonstrationBuffer(vae, ppo, capacity, chunk=64) is the warm start in front of all this: behaviour cloning from (camera frame, measurements, expert action[, return])
rows -- CARLA's autopilot, a human driver.  add() encodes the frames with the batched recording step (greedy, at most `chunk` per call) into a device table of
state rows, clone() runs epochs of shuffled minibatches through PPO._clone_rows (mi_ppo_clone_step: the fused chain with a supervised head / loss kernel, loss "nll"
or "mse"; the value net is fitted if and only if returns were added, and is otherwise neither run nor touched), evaluate() scores the policy against the expert in
float64 on the host.  Single rank; no latent stacking.

RolloutBuffer.set_demonstrations(demo_buffer, coef, loss="nll", batch_size=32, decay=1.0, seed=0) keeps the demonstrations in the PPO update behind the warm start
(DAPG; a warm-started policy beside a value net that has seen no on-policy data is where the first PPO updates undo the warm start): with it on, every SGD step of
update() / update_with_diagnostics() is ONE PPO._demo_rows call (mi_ppo_train_step_demo) on the PPO minibatch plus min(batch_size, demo_buffer.size) demonstration
rows -- loss = L_ppo + coef x clone_loss(those rows), one fused chain over all rows, one gradient, one Adam update; value clipping and the KL penalty apply to the PPO
rows, the demonstration rows carry no value target.  The demonstration rows come from a np.random.RandomState(seed) the setting owns (a permutation of the rows and a
cursor; when fewer rows than a minibatch remain a fresh permutation is drawn: demonstration_rows_drawn), so the legacy numpy stream that shuffles the PPO minibatches is
consumed exactly as with the setting off.  After every update coef *= decay; demonstration_state() / load_demonstration_state() carry the coefficient, the
RandomState, the permutation and the cursor.  The result gains `demo_losses` (one {demo_loss, mean_sq_error} per step), `demo_rows`, `demo_coef` and `demo_coef_next`;
with the setting off no key appears and the update makes the launches it always made.  Refused before anything is launched: an empty demonstration buffer, another
input_dim / action count / ppo object, a stacked rollout buffer, observation normalisation that is not off in both buffers or frozen here and equal by value to the
state the demonstration buffer was given, and a policy outside the fused kernels' range.

RolloutBuffer.set_advantage_recomputation(on=True) RECOMPUTES VALUES AND ADVANTAGES before every epoch of an update but the first (Andrychowicz et al. 2021, "What
Matters in On-Policy RL": by epoch 2 the value net has moved, and returns and advantages formed from the values of collection time are stale).  Epoch 1 is the epoch
it always was -- the finish call reads the recorded `values` -- so num_epochs = 1 is bitwise the setting off.  Before every later epoch that runs (a KL stop ends the
refreshes with the epochs) the stage "recompute" makes ONE mi_ppo_values_idx call (the value net alone, forward only, chunked inside the entry) over the recorded rows
and the bootstrap slots of `states` into a second table `values_now`, and repeats the update's finish call with `values_now` in the place of `values` and everything
else as it was; `returns` and `advantages`, which the steps gather from, are rewritten, and per-minibatch normalisation reads the refreshed raw advantages.  `values`
stays the collection-time table: value clipping reads it as V_old (PPO2's meaning) and `out["values"]` returns it; `returns` / `advantages` / `raw_advantages` of the
result are the first finish call's.  New keys: `recomputed_epochs`, and when a refresh ran `refreshed_values` (fp32) and `refreshed_returns` /
`refreshed_advantages` / `refreshed_raw_advantages` (fp64), [num_envs, T] of the LAST refresh, NaN beyond a lane's length.  ContinuousRolloutBuffer.truncate() becomes
a greedy recording call that keeps the final observation's state row in `final_states`; every refresh values those rows into `final_values_now`, from which the
truncated segments then bootstrap; `final_values` stays the recorded table and the result gains `refreshed_final_values`.  Needs the fused kernels; switched only
with no step recorded.  With the setting off no table is allocated and every call makes the launches it always made.

RolloutBuffer.set_vtrace(rho_bar=1.0, c_bar=1.0) puts V-TRACE OFF-POLICY CORRECTION on those refreshes (Espeholt et al. 2018, IMPALA): by epoch 2 the policy has moved
away from the one that drew the recorded actions, and plain GAE on the refreshed values estimates the wrong quantity.  With it on a refresh is the values_idx call, ONE
mi_ppo_logp_idx call (the policy net alone, forward only) over the recorded rows of `states` / `actions` into a table `logp_now`, and mi_rollout_finish_vtrace on
`values_now`, `logp_now` and the update's cache of log pi_old in the place of the GAE finish call: w = exp(logp_now - logp_old) per step, min(rho_bar, w) on the TD errors
and lam min(c_bar, w) on the trace; the returns are the V-trace value targets and the advantages delta_t + gamma lam (vs_{t+1} - V_{t+1}), normalised as the update
normalises.  Same rewards, dones, segments, gamma, lam and truncation source as the GAE refresh; RolloutBuffer keeps mi_rollout_finish's successor-value rule,
ContinuousRolloutBuffer the segment kernels'.  The first finish call stays the GAE call (theta == theta_old there and V-trace equals it bit for bit), the SGD steps still
read the collection-time cache of log pi_old.  New keys, from the last refresh that ran: `refreshed_importance_weights` (fp64 [num_envs, T], NaN beyond a lane's length),
`vtrace_rho_clip_fraction` and `vtrace_c_clip_fraction` (the share of recorded steps whose weight exceeds the bar).  update() refuses V-trace without advantage
recomputation or without the fused kernels; set_vtrace(None) turns it off, bitwise a buffer that never had it.
"""
import contextlib
import numbers
import os
import time
import types

import numpy as np

from mi355 import lib as milib


MAX_ENVS = 1024                                                                      # MI_ROLLOUT_MAX_ENVS of include/mi355_carla.h
MAX_STACK = 16                                                                       # MI_ROLLOUT_MAX_STACK
MAX_STACK_INPUTS = 1024                                                              # the widest state rollout_stack_kernel assembles (and PPO.set_wide_inputs() trains)


def latent_stack_checked(latent_stack, z_dim, input_dim, who):
    """The checked `latent_stack` of a step class or buffer -> (k, n_meas): an int in [1, MAX_STACK] with k z_dim <= input_dim and, for k > 1, at most
    MAX_STACK_INPUTS inputs.  ValueError otherwise.  No device and no library involved."""
    k = latent_stack
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_STACK:
        raise ValueError("%s: latent_stack is an int in [1, %d], got %r" % (who, MAX_STACK, k))
    k, z_dim, input_dim = int(k), int(z_dim), int(input_dim)
    if k * z_dim > input_dim:
        raise ValueError("the policy takes fewer inputs than the VAE's latent size" if k == 1 else
                         "%s: latent_stack = %d latents of %d are %d inputs, the policy takes %d" % (who, k, z_dim, k * z_dim, input_dim))
    if k > 1 and input_dim > MAX_STACK_INPUTS:
        raise ValueError("%s: latent_stack = %d gives a state of %d inputs, the stacked step assembles at most %d" % (who, k, input_dim, MAX_STACK_INPUTS))
    return k, input_dim - k * z_dim


def latent_history_state_checked(d, k, z_dim, num_envs, who):
    """The checked dict of history_state() for a step of `num_envs` lanes, latent_stack = k and latents of z_dim -> {"history": float32 [num_envs, k - 1, z_dim],
    "fresh": bool [num_envs]}.  ValueError otherwise.  numpy only."""
    keys = ("latent_stack", "z_dim", "history", "fresh")
    if not isinstance(d, dict) or any(key not in d for key in keys):
        raise ValueError("%s: expected a dict with the keys %s" % (who, ", ".join(keys)))
    for key, want in (("latent_stack", k), ("z_dim", z_dim)):
        got = d[key]
        if isinstance(got, (bool, np.bool_)) or not isinstance(got, (int, np.integer)) or int(got) != want:
            raise ValueError("%s: the state was taken with %s = %r, this one has %d" % (who, key, got, want))
    h, f = np.asarray(d["history"]), np.asarray(d["fresh"])
    if h.dtype.kind != "f" or h.shape != (num_envs, k - 1, z_dim):
        raise ValueError("%s: history must be floats of shape (%d, %d, %d), got %s %s" % (who, num_envs, k - 1, z_dim, h.dtype, h.shape))
    if f.dtype.kind != "b" or f.shape != (num_envs,):
        raise ValueError("%s: fresh must be bools of shape (%d,), got %s %s" % (who, num_envs, f.dtype, f.shape))
    return {"history": np.ascontiguousarray(h, np.float32), "fresh": f.copy()}


class _StepBase:
    """What every step class starts from: the engines' handles, the sizes, the io mode and the Philox noise stream."""

    def _setup(self, who, vae, ppo, seed, io, latent_stack=1):
        """-> (the VAE's device engine, the policy's)."""
        self.vae, self.ppo = vae, ppo
        self.z_dim, self.A = int(vae.z_dim), int(ppo.num_actions)
        self.k, self.n_meas = latent_stack_checked(latent_stack, self.z_dim, ppo.input_dim, getattr(self, "_who", who))      # (raises before anything touches a device)
        self.latent_cols, self.din = self.k * self.z_dim, self.k * self.z_dim + self.n_meas            # the state's latent columns: what normalize_latents=False is about
        vdev, pdev = vae._need_dev(), ppo._need_dev()
        self.L = vdev.L
        self.device = vdev.device
        self.io = io or os.environ.get("MI355_ROLLOUT_IO", "pinned")
        if self.io not in ("pinned", "device"):
            raise ValueError(who + ": io must be 'pinned' or 'device'")
        self.frame_bytes = int(np.prod(vdev.source_shape))
        self._rng = np.random.Generator(np.random.Philox(int(seed if seed is not None else (ppo.seed or 0)) + 0xAC7))
        self._obs_norm = None                                                        # running observation normalisation (set_observation_normalization): None = off
        self._kind = getattr(vdev, "rollout_kind", "conv")                           # "mlp": an MlpVaeDevice, whose handle goes to the mi_mlp_rollout_* entries alone
        if self._kind not in ("conv", "mlp"):
            raise ValueError(who + ": unknown encoder kind %r" % (self._kind,))
        return vdev, pdev

    def _io_buffers(self, in_bytes, out_floats):
        """Pinned host buffers, and their device twins for io="device" (one copy each way per call)."""
        import torch
        self.h_in = torch.empty(in_bytes, dtype=torch.uint8).pin_memory()
        self.h_out = torch.empty(out_floats, dtype=torch.float32).pin_memory()
        dev_io = self.io == "device"
        self.d_in = torch.empty(in_bytes, dtype=torch.uint8, device=self.device) if dev_io else None
        self.d_out = torch.empty(out_floats, dtype=torch.float32, device=self.device) if dev_io else None
        self._in_np = self.h_in.numpy()


class RolloutStep(_StepBase):
    def __init__(self, vae, ppo, seed=None, io=None):
        self._setup("RolloutStep", vae, ppo, seed, io)
        if self._kind != "conv":                                                     # (mi_rollout_step would read the MLP engine as a ConvVAE engine)
            raise ValueError("RolloutStep: the single-frame entry exists for the ConvVAE only: use BatchedRolloutStep(vae, ppo, num_envs=1)")
        self._noise_off = (self.frame_bytes + 15) // 16 * 16                         # float region: measurements, then noise
        self._io_buffers(self._noise_off + 4 * (self.n_meas + self.A), self.A + 1 + self.z_dim)
        self._f_np = self._in_np[self._noise_off:].view(np.float32)
        self._out_np = self.h_out.numpy()

    @classmethod
    def stacked(cls, vae, ppo, latent_stack, seed=None, io=None):
        """The single-frame entry has no stacked form: ValueError for anything but latent_stack = 1."""
        if isinstance(latent_stack, (bool, np.bool_)) or not isinstance(latent_stack, (int, np.integer)) or int(latent_stack) != 1:
            raise ValueError("RolloutStep: latent stacking exists in the batched step only: use BatchedRolloutStep.stacked(vae, ppo, num_envs=1, latent_stack=k)")
        return cls(vae, ppo, seed=seed, io=io)

    def set_observation_normalization(self, state_dict):
        """The single-frame entry has no normalised form: ValueError for anything but None."""
        if state_dict is not None:
            raise ValueError("RolloutStep: observation normalisation exists in the batched step only: use BatchedRolloutStep(vae, ppo, num_envs=1)")

    def __call__(self, frame_u8, measurements, greedy=False, noise=None):
        """frame_u8: uint8 [H, W, 3] camera frame; measurements: the k values appended to the latent.  Returns (action [A], value, state [z + k])."""
        import torch
        f = np.asarray(frame_u8)
        if f.dtype != np.uint8 or f.size != self.frame_bytes:
            raise ValueError("RolloutStep: expected a uint8 frame of %d bytes" % self.frame_bytes)
        meas = np.asarray(measurements, np.float64).reshape(-1)
        if meas.size != self.n_meas:
            raise ValueError("RolloutStep: expected %d measurements" % self.n_meas)
        self._in_np[:self.frame_bytes] = f.reshape(-1)
        self._f_np[:self.n_meas] = meas                                              # f64 -> f32 at the feed, as ppo.py:108-109
        if not greedy:
            self._f_np[self.n_meas:] = self._rng.standard_normal(self.A) if noise is None else np.asarray(noise, np.float32).reshape(self.A)
        st = torch.cuda.current_stream(self.device)
        if self.d_in is not None:
            self.d_in.copy_(self.h_in, non_blocking=True)
        base = (self.h_in if self.d_in is None else self.d_in).data_ptr()
        fptr = base + self._noise_off
        self.L.mi_rollout_step(self.vae.dev.handle, self.ppo.dev.handle, st.cuda_stream, base, fptr, self.n_meas,
                               None if greedy else fptr + 4 * self.n_meas, 1 if greedy else 0, (self.h_out if self.d_out is None else self.d_out).data_ptr())
        if self.d_out is not None:
            self.h_out.copy_(self.d_out, non_blocking=True)
        st.synchronize()
        o = self._out_np
        action, value = o[:self.A].copy(), float(o[self.A])
        state = np.append(o[self.A + 1:].copy(), meas)                               # float64, like np.append(float32[z], python floats)
        return action, value, state


class BatchedRolloutStep(_StepBase):
    """RolloutStep for up to `num_envs` environments per call (mi_rollout_step_batch): frames_u8 [n, H, W, 3] uint8 and measurements [n, k] in,
    (actions float32 [n, A], values float32 [n], states float64 [n, z_dim + k]) out, 1 <= n <= num_envs -- environments finish their episodes at
    different times.  Row e is what RolloutStep gives for frame e: np.append(vae.encode([frame_e])[0], meas_e) and model.predict of it.  With an MlpVAE every device
    call is mi_mlp_rollout_step_batch / mi_mlp_rollout_value_batch instead (one entry each for the plain, recording and normalised forms)."""

    _who = "BatchedRolloutStep"                                                      # the prefix of check()'s messages
    _row_ints = 0                                                                    # int32 per environment behind the noise (the recording step's table rows)

    def __init__(self, vae, ppo, num_envs, seed=None, io=None):
        self._init(vae, ppo, num_envs, seed, io, 1)

    @classmethod
    def stacked(cls, vae, ppo, num_envs, latent_stack, seed=None, io=None):
        """The step with LATENT STACKING (see the module docstring): cls(vae, ppo, num_envs, seed, io) whose state is [z_t | the latent_stack - 1 latents before it |
        measurements], from a device-resident `history` [num_envs, latent_stack - 1, z_dim] the step owns.  latent_stack: an int in [1, 16] (1: the plain step) with
        latent_stack x z_dim <= the policy's input size <= 1024; ValueError otherwise, before anything touches a device."""
        self = cls.__new__(cls)                                                      # (not cls(..): a subclass that needs more than these arguments overrides _init, as the buffers do)
        self._init(vae, ppo, num_envs, seed, io, latent_stack)
        return self

    def _init(self, vae, ppo, num_envs, seed, io, latent_stack):
        import torch
        self.num_envs = int(num_envs)
        if not 1 <= self.num_envs <= MAX_ENVS:
            raise ValueError("BatchedRolloutStep: 1 <= num_envs <= %d" % MAX_ENVS)
        vdev, pdev = self._setup("BatchedRolloutStep", vae, ppo, seed, io, latent_stack)
        pdev.ensure_batch(self.num_envs)                                             # recreates the engine when it grows: ppo.dev.handle is read per call
        E, self.row = self.num_envs, self.A + 1 + self.z_dim
        self._f_off = (E * self.frame_bytes + 15) // 16 * 16                         # float region: measurements [E, k], then noise [E, A], then _row_ints [E]
        stacked = self.k > 1                                                         # latent stacking: lanes and fresh flags [E] behind the table rows, the older latents behind the output rows
        self._older_off = E * self.row
        self._io_buffers(self._f_off + 4 * E * (self.n_meas + self.A + self._row_ints + (2 if stacked else 0)), E * (self.row + (self.k - 1) * self.z_dim))
        if stacked:
            self.history = torch.zeros(E, self.k - 1, self.z_dim, device=self.device)
            self.fresh = np.ones(E, bool)
            self.sstate = torch.empty(E, self.din, device=self.device)
        if self._kind == "mlp":                                                      # sized from the descriptor: no handle involved
            import ctypes
            entry, self.scratch_bytes = "mi_mlp_rollout_workspace_bytes", int(self.L.mi_mlp_rollout_workspace_bytes(ctypes.byref(vdev._desc(1)), E))
        else:
            entry, self.scratch_bytes = "mi_rollout_batch_workspace_bytes", int(self.L.mi_rollout_batch_workspace_bytes(vae.dev.handle, ppo.dev.handle, E))
        if self.scratch_bytes <= 0:
            raise milib.MiError(entry + ": " + self.L.cdll.mi_last_error().decode())
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=self.device)
        self._f_np = self._in_np[self._f_off:].view(np.float32)
        self._i_np = self._in_np[self._f_off:].view(np.int32)
        self._out_np = self.h_out.numpy()[:E * self.row].reshape(E, self.row)
        self._older_np = self.h_out.numpy()[E * self.row:]

    def __call__(self, frames_u8, measurements, greedy=False, noise=None):
        return self.record(*self.check(frames_u8, measurements, greedy, noise), greedy)

    def step(self, frames_u8, measurements, env_ids=None, greedy=False, noise=None):
        """__call__ with the environment of every row, in the buffers' argument order: env_ids (None: 0 .. n-1, what __call__ takes) are the history lanes of the rows --
        read with latent stacking on only, checked whenever given (distinct, inside [0, num_envs): ValueError otherwise)."""
        f, n, meas, nz = self.check(frames_u8, measurements, greedy, noise)
        return self.record(f, n, meas, nz, greedy, lanes=None if env_ids is None else self.lanes_checked(env_ids, n))

    def lanes_checked(self, env_ids, n):
        """env_ids (None: 0 .. n-1) of a call with n rows -> int64 [n], distinct, inside [0, num_envs).  ValueError otherwise."""
        if env_ids is None:
            return np.arange(n, dtype=np.int64)
        ids = np.asarray(env_ids)
        if ids.ndim != 1 or ids.dtype.kind not in "iu" or ids.shape[0] != n:
            raise ValueError("%s: env_ids must be a vector of %d integers" % (self._who, n))
        ids = ids.astype(np.int64)
        if ids.min() < 0 or ids.max() >= self.num_envs:
            raise ValueError("%s: env_ids outside [0, %d)" % (self._who, self.num_envs))
        if np.unique(ids).shape[0] != n:
            raise ValueError("%s: duplicate env_ids" % self._who)
        return ids

    def _need_stack(self, what):
        if self.k < 2:
            raise ValueError("%s.%s: latent stacking is off (build it with stacked(.., latent_stack=k))" % (self._who, what))

    def restart(self, env_ids=None):
        """These lanes (None: all) start an episode with their next call: its row repeats its own latent and the lane's old history is never read."""
        self._need_stack("restart")
        if env_ids is None:
            self.fresh[:] = True
        else:
            ids = np.asarray(env_ids)
            self.fresh[self.lanes_checked(ids, ids.shape[0] if ids.ndim == 1 else -1)] = True

    def history_state(self):
        """What a training script writes to its checkpoint: {"latent_stack", "z_dim", "history": float32 [num_envs, latent_stack - 1, z_dim], "fresh": bool [num_envs]}."""
        self._need_stack("history_state")
        return {"latent_stack": self.k, "z_dim": self.z_dim, "history": self.history.cpu().numpy(), "fresh": self.fresh.copy()}

    def load_history_state(self, d):
        """Takes history_state()'s dict back.  The whole dict is checked before anything changes (ValueError)."""
        import torch
        self._need_stack("load_history_state")
        d = latent_history_state_checked(d, self.k, self.z_dim, self.num_envs, self._who + ".load_history_state")
        self.history.copy_(torch.from_numpy(d["history"]))
        self.fresh[:] = d["fresh"]

    def set_observation_normalization(self, state_dict):
        """The FROZEN evaluation step: a checkpointed observation_normalization_state() of a buffer (None: off) is applied by every call from now on
        (mi_rollout_step_batch_norm with table_rows = NULL) and never updated.  The whole dict is checked before anything changes (ValueError).  The states a call
        returns stay the raw observation."""
        if state_dict is None:
            self._obs_norm = None
            return
        who = self._who + ".set_observation_normalization"
        d = observation_normalization_state_checked(state_dict, self.din, who)
        settings = _obs_norm_settings_of(d, self.latent_cols, who, "step")
        on = _obs_norm_tensors(self.device, self.din, self.num_envs)
        on.update(settings)
        _obs_norm_load(self.L, on, d, self.latent_cols)
        self._obs_norm = on

    def check(self, frames_u8, measurements, greedy, noise):
        """The host-side checks of a call -> (frames, n, measurements float64 [n, k], noise float32 [n, A] or None)."""
        f = np.asarray(frames_u8)
        if f.dtype != np.uint8 or f.ndim < 1 or f.size != f.shape[0] * self.frame_bytes:
            raise ValueError("%s: expected uint8 frames [n, ...] of %d bytes each" % (self._who, self.frame_bytes))
        n = int(f.shape[0])
        if not 1 <= n <= self.num_envs:
            raise ValueError("%s: 1 <= n <= num_envs = %d, got %d" % (self._who, self.num_envs, n))
        meas = np.asarray(measurements, np.float64)
        if meas.shape != (n, self.n_meas):
            raise ValueError("%s: expected measurements [%d, %d]" % (self._who, n, self.n_meas))
        nz = None
        if not greedy and noise is not None:
            nz = np.asarray(noise, np.float32)
            if nz.shape != (n, self.A):
                raise ValueError("%s: expected noise [%d, %d]" % (self._who, n, self.A))
        return f, n, meas, nz

    # (class attributes, as defaults of what _setup() sets: the host tests' stub steps -- tests/test_mlp_rollout_host.py, test_observation_normalization_host.py,
    # test_rollout_update_sequence_host.py -- are built without _setup() and carry none of its attributes: they are the ConvVAE step without stacking)
    k, _kind = 1, "conv"

    def _stage(self, f, n, meas, na, noise, table_rows, lanes):
        """Stages the input of one device call: the frames, the measurements, the noise block of na floats (noise None: left as it is, the greedy step) and the int32
        blocks behind it -- the table rows (None: none) and, with latent stacking on, the lanes (None: 0 .. n-1) and their fresh flags -- go into the pinned buffer,
        and from there to the device where the io mode has a device buffer.  -> (stream, base, fptr, rows_ptr, lanes_ptr, lanes): the addresses of the frames, of the measurements (the noise lies 4 n n_meas bytes
        behind), of the table rows and of the lanes (the fresh flags lie 4 n bytes behind)."""
        import torch
        self._in_np[:n * self.frame_bytes] = f.reshape(-1)
        o = n * self.n_meas
        self._f_np[:o] = meas.reshape(-1)                                            # f64 -> f32 at the feed, as ppo.py:108-109
        if noise is not None:
            self._f_np[o:o + na] = noise.reshape(-1)
        o += na
        rows_off = o
        if table_rows is not None:
            self._i_np[o:o + n] = table_rows
            o += n
        lanes_off = o
        if self.k > 1:
            lanes = np.arange(n) if lanes is None else lanes
            self._i_np[o:o + n] = lanes
            self._i_np[o + n:o + 2 * n] = self.fresh[lanes]
            o += 2 * n
        st = torch.cuda.current_stream(self.device)
        used = self._f_off + 4 * o
        if self.d_in is not None:
            self.d_in[:used].copy_(self.h_in[:used], non_blocking=True)
        base = (self.h_in if self.d_in is None else self.d_in).data_ptr()
        fptr = base + self._f_off
        return st, base, fptr, fptr + 4 * rows_off, fptr + 4 * lanes_off, lanes

    def _norm_args(self, nstate):
        """obs_mean, obs_inv_std, obs_clip [, nstate] of an entry: NULLs and 0.0 with observation normalisation off."""
        on = self._obs_norm
        args = (None, None, 0.0, None) if on is None else (on["mean32"].data_ptr(), on["inv32"].data_ptr(), on["clip"], on["nstate"].data_ptr())
        return args if nstate else args[:3]

    def _fetch(self, st, *ranges):
        """The call's output in the host buffer: the copy of these [lo, hi) of the output buffer where the io mode has a device buffer, and the wait for the stream."""
        if self.d_out is not None:
            for lo, hi in ranges:
                self.h_out[lo:hi].copy_(self.d_out[lo:hi], non_blocking=True)
        st.synchronize()

    def record(self, f, n, meas, nz, greedy, table_rows=None, states=None, actions=None, values=None, raw_states=None, lanes=None, advance=True):
        """One device call on checked inputs.  table_rows None: mi_rollout_step_batch; else the int32 table rows go behind the noise and mi_rollout_step_batch_rec also
        leaves state / action / value of row i in row table_rows[i] of the device tables `states`, `actions`, `values`.  With observation normalisation on
        (set_observation_normalization) either becomes mi_rollout_step_batch_norm: `states` then takes the normalised rows and `raw_states` the raw ones.
        With latent stacking on every form is mi_rollout_step_batch_stack: `lanes` (None: 0 .. n-1) and their fresh flags go behind the table rows, the lanes' history
        advances unless `advance` is False, and the lanes are no longer fresh afterwards."""
        noise = None if greedy else (self._rng.standard_normal((n, self.A)) if nz is None else nz)
        st, base, fptr, rows_ptr, lanes_ptr, lanes = self._stage(f, n, meas, n * self.A, noise, table_rows, lanes)
        out = (self.h_out if self.d_out is None else self.d_out).data_ptr()
        args = (self.vae.dev.handle, self.ppo.dev.handle, st.cuda_stream, base, fptr, self.n_meas, None if greedy else fptr + 4 * n * self.n_meas, 1 if greedy else 0, n,
                self.scratch.data_ptr(), self.scratch_bytes, out)
        on, stacked, mlp = self._obs_norm, self.k > 1, self._kind == "mlp"
        if table_rows is None:                                                       # table_rows NULL = nothing recorded
            tabs = (None, 0, None, None, None, None)
        else:
            tabs = (rows_ptr, int(states.shape[0]), states.data_ptr(), None if on is None else raw_states.data_ptr(), actions.data_ptr(), values.data_ptr())
        if stacked:                                                                  # one entry per encoder: obs_mean NULL = not normalised
            entry = self.L.mi_mlp_rollout_step_batch_stack if mlp else self.L.mi_rollout_step_batch_stack
            entry(*args, *self._norm_args(False), *tabs, self.k, self.history.data_ptr(), self.num_envs, lanes_ptr, lanes_ptr + 4 * n, 1 if advance else 0,
                  self.sstate.data_ptr(), out + 4 * self._older_off)
        elif mlp:                                                                    # one entry: obs_mean NULL = not normalised
            self.L.mi_mlp_rollout_step_batch(*args, *self._norm_args(True), *tabs)
        elif on is not None:
            self.L.mi_rollout_step_batch_norm(*args, *self._norm_args(True), *tabs)
        elif table_rows is None:
            self.L.mi_rollout_step_batch(*args)
        else:
            self.L.mi_rollout_step_batch_rec(*args, *tabs[:3], *tabs[4:])             # (no raw table without normalisation)
        n_older = n * (self.k - 1) * self.z_dim
        self._fetch(st, (0, n * self.row), *([(self._older_off, self._older_off + n_older)] if stacked else []))
        o = self._out_np[:n]
        if not stacked:
            return o[:, :self.A].copy(), o[:, self.A].copy(), np.concatenate([o[:, self.A + 1:].astype(np.float64), meas], axis=1)
        if advance:
            self.fresh[lanes] = False
        older = self._older_np[:n_older].reshape(n, -1)                              # the raw row the kernel assembled: [z_t | the older latents | measurements]
        return o[:, :self.A].copy(), o[:, self.A].copy(), np.concatenate([o[:, self.A + 1:], older, meas.astype(np.float32)], axis=1).astype(np.float64)      # (the measurements as the kernel read them: fp32)

    def record_value(self, f, n, meas, table_rows, final_values):
        """The value-only device call on checked inputs (mi_rollout_value_batch_rec; with observation normalisation on, mi_rollout_value_batch_norm: the encoder chain,
        the value trunk and the value head; no action, no latent comes back): the int32 table rows go behind the measurements and the value of row i is also left in final_values[table_rows[i]].  -> float32 [n]."""
        return self.record_value_lanes(f, n, meas, table_rows, final_values, None)

    def record_value_lanes(self, f, n, meas, table_rows, final_values, lanes):
        """record_value() with the history lanes of the rows (None: 0 .. n-1), which are read with latent stacking on only: the call is then
        mi_rollout_value_batch_stack, which values the observation on its lane's history and never advances it."""
        st, base, fptr, rows_ptr, lanes_ptr, lanes = self._stage(f, n, meas, 0, None, table_rows, lanes)
        args = (self.vae.dev.handle, self.ppo.dev.handle, st.cuda_stream, base, fptr, self.n_meas, n, self.scratch.data_ptr(), self.scratch_bytes,
                (self.h_out if self.d_out is None else self.d_out).data_ptr())
        rec = (rows_ptr, int(final_values.shape[0]), final_values.data_ptr())
        mlp = self._kind == "mlp"
        if self.k > 1:                                                               # latent stacking: the history is read, never advanced
            entry = self.L.mi_mlp_rollout_value_batch_stack if mlp else self.L.mi_rollout_value_batch_stack
            entry(*args, *self._norm_args(False), *rec, self.k, self.history.data_ptr(), self.num_envs, lanes_ptr, lanes_ptr + 4 * n, self.sstate.data_ptr())
        elif mlp:
            self.L.mi_mlp_rollout_value_batch(*args, *self._norm_args(True), *rec)
        elif self._obs_norm is not None:
            self.L.mi_rollout_value_batch_norm(*args, *self._norm_args(True), *rec)
        else:
            self.L.mi_rollout_value_batch_rec(*args, *rec)
        self._fetch(st, (0, n))
        return self.h_out.numpy()[:n].copy()


MAX_HORIZON = 4096                                                                   # MI_ROLLOUT_MAX_HORIZON of include/mi355_carla.h


class RolloutRows:
    """The row book-keeping of a RolloutBuffer; numpy only (no torch, no GPU).  Environment e owns the table rows e (horizon + 1) .. e (horizon + 1) + horizon.  A row is
    open (it takes steps), awaiting the outcome of its last recorded step, ended (its environment reported done or it is full: it takes the bootstrap only) or closed
    (bootstrapped).  Every method checks its whole call before it changes anything and raises ValueError."""

    def __init__(self, num_envs, horizon):
        self.num_envs, self.horizon = int(num_envs), int(horizon)
        if not 1 <= self.num_envs <= MAX_ENVS:
            raise ValueError("RolloutBuffer: 1 <= num_envs <= %d" % MAX_ENVS)
        if not 1 <= self.horizon <= MAX_HORIZON:
            raise ValueError("RolloutBuffer: 1 <= horizon <= %d" % MAX_HORIZON)
        self._all = np.arange(self.num_envs, dtype=np.int64)
        self._base = (self._all * (self.horizon + 1)).astype(np.int32)               # table row of slot 0 of every environment
        self.reset()

    OPEN, AWAITING, ENDED, CLOSED = 0, 1, 2, 3                                        # per row, one small array: a call is a handful of numpy operations

    def reset(self):
        E, T = self.num_envs, self.horizon
        self.lengths = np.zeros(E, np.int32)
        self.state = np.zeros(E, np.int8)
        self.rewards, self.dones = np.zeros((E, T), np.float64), np.zeros((E, T), np.float64)

    @property
    def awaiting(self):
        """A step is recorded at slot lengths[e]; its reward / done are not in yet."""
        return self.state == self.AWAITING

    @property
    def ended(self):
        """done was reported or the horizon is reached: no further step, the bootstrap only."""
        return self.state == self.ENDED

    @property
    def closed(self):
        return self.state == self.CLOSED

    def env_ids(self, env_ids, n):
        """env_ids (None = 0 .. n-1) of a call with n rows -> int64 [n], distinct, inside [0, num_envs)."""
        if env_ids is not None:
            ids = np.asarray(env_ids)
            if ids.ndim != 1 or ids.dtype.kind not in "iu":
                raise ValueError("RolloutBuffer: env_ids must be a vector of integers")
            ids = ids.astype(np.int64)
            if ids.shape[0] != n:
                raise ValueError("RolloutBuffer: %d env_ids for %d rows" % (ids.shape[0], n))
        if n < 1 or n > self.num_envs:
            raise ValueError("RolloutBuffer: 1 <= n <= num_envs = %d, got %d" % (self.num_envs, n))
        if env_ids is None:                                                          # 0 .. n-1: distinct and in range once n is
            return self._all[:n]
        if ids.min() < 0 or ids.max() >= self.num_envs:
            raise ValueError("RolloutBuffer: env_ids outside [0, %d)" % self.num_envs)
        if np.unique(ids).shape[0] != n:
            raise ValueError("RolloutBuffer: duplicate env_ids")
        return ids

    def _rows(self, ids):
        return self._base[ids] + self.lengths[ids]                                   # int32

    def _refuse(self, what, ids, st, codes):
        for code, why in codes:
            if (st == code).any():
                raise ValueError("RolloutBuffer: %s %s (environments %s)" % (what, why, ids[st == code].tolist()))

    def step_rows(self, env_ids, n):
        """The table rows a step of these environments records into; marks them as awaiting their outcome."""
        ids = self.env_ids(env_ids, n)
        st = self.state[ids]
        if st.any():
            self._refuse("step on", ids, st, ((self.CLOSED, "a closed row"), (self.AWAITING, "a row whose last step has no outcome yet"),
                                              (self.ENDED, "a full row -- done was reported or the horizon is reached")))
        rows = self._rows(ids)
        self.state[ids] = self.AWAITING
        return rows

    def outcome(self, rewards, dones, env_ids=None):
        """Reward and done of the step just recorded for these environments: the step now counts."""
        r = np.asarray(rewards, np.float64)
        d = np.asarray(dones)
        if r.ndim != 1 or d.shape != r.shape:
            raise ValueError("RolloutBuffer: rewards and dones must be vectors of one length")
        ids = self.env_ids(env_ids, r.shape[0])
        st = self.state[ids]
        if (st != self.AWAITING).any():
            raise ValueError("RolloutBuffer: outcome without a recorded step (environments %s)" % ids[st != self.AWAITING].tolist())
        slot = self.lengths[ids]
        self.rewards[ids, slot], self.dones[ids, slot] = r, d
        self.lengths[ids] = slot + 1
        self.state[ids] = np.where(self._ends(d.astype(bool), slot + 1), self.ENDED, self.OPEN)

    def _ends(self, done, length):
        """Does a row whose step just counted take no further step?  done was reported, or the horizon is reached."""
        return done | (length >= self.horizon)

    def bootstrap_rows(self, env_ids, n):
        """The table rows (slot lengths[e]) that take the state after the last step and its value; closes the rows."""
        ids = self.env_ids(env_ids, n)
        st = self.state[ids]
        self._refuse("bootstrap of", ids, st, ((self.CLOSED, "a closed row"), (self.AWAITING, "a row whose last step has no outcome yet")))
        if (self.lengths[ids] < 1).any():
            raise ValueError("RolloutBuffer: bootstrap of an empty row (environments %s)" % ids[self.lengths[ids] < 1].tolist())
        rows = self._rows(ids)
        self.state[ids] = self.CLOSED
        return rows

    def stepped(self):
        """Environments with a non-empty row that is not closed yet (the default of RolloutBuffer.bootstrap)."""
        return np.nonzero((self.lengths > 0) & (self.state != self.CLOSED))[0]

    def check_update(self):
        open_rows = np.nonzero(((self.lengths > 0) | (self.state == self.AWAITING)) & (self.state != self.CLOSED))[0]
        if open_rows.size:
            raise ValueError("RolloutBuffer: update with open rows (environments %s): bootstrap them first" % open_rows.tolist())
        if int(self.lengths.sum()) < 1:
            raise ValueError("RolloutBuffer: update with no samples")

    def valid_rows(self):
        """Table rows of all recorded steps: rows in environment order, slots ascending (int32)."""
        T1 = self.horizon + 1
        parts = [e * T1 + np.arange(self.lengths[e]) for e in range(self.num_envs)]
        return np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)


class SegmentedRows(RolloutRows):
    """RolloutRows for lanes that hold SEVERAL episodes (ContinuousRolloutBuffer): a done does not end a lane, the next step of that environment records at slot
    lengths[e] and starts a new segment; a lane is ended only when it is full.  A segment is a maximal run of recorded steps of a lane that ends at a step with
    done != 0, at a TRUNCATED step or at the lane's last recorded step; only a lane's last segment can end without either, and slot lengths[e] behind it is the lane's
    bootstrap slot.  A truncated step (truncate_rows) is the last step of an episode that stopped without being terminal -- a step or time limit, a restarted simulator,
    a route switch -- and is followed by a reset in the same lane: its segment bootstraps from the value of the episode's final observation, which is no step of the
    lane and is kept beside the step's own row (ContinuousRolloutBuffer.final_values)."""

    def reset(self):
        super().reset()
        self.truncs = np.zeros((self.num_envs, self.horizon), bool)

    def _ends(self, done, length):
        return length >= self.horizon

    def _last_done(self):
        """Per lane: its last counted step reported done or was truncated -- nothing behind it is read (False for an empty lane)."""
        last = np.maximum(self.lengths, 1) - 1
        return (self.lengths > 0) & ((self.dones[self._all, last] != 0) | self.truncs[self._all, last])

    def truncate_rows(self, env_ids, n):
        """The table rows of the last counted step (slot lengths[e] - 1) of these lanes; marks the steps as truncated.  The lanes go on as they were: an open lane takes
        its next step (the reset observation), a full one needs no bootstrap any more."""
        ids = self.env_ids(env_ids, n)
        st = self.state[ids]
        self._refuse("truncation of", ids, st, ((self.CLOSED, "a closed row"), (self.AWAITING, "a row whose last step has no outcome yet")))
        if (self.lengths[ids] < 1).any():
            raise ValueError("RolloutBuffer: truncation of an empty row (environments %s)" % ids[self.lengths[ids] < 1].tolist())
        last = self.lengths[ids] - 1
        if (self.dones[ids, last] != 0).any():
            raise ValueError("RolloutBuffer: truncation of a row whose last step reported done -- a terminal stays a terminal (environments %s)"
                             % ids[self.dones[ids, last] != 0].tolist())
        if self.truncs[ids, last].any():
            raise ValueError("RolloutBuffer: truncation of a row whose last step is already truncated (environments %s)" % ids[self.truncs[ids, last]].tolist())
        self.truncs[ids, last] = True
        return self._base[ids] + last                                                # int32

    def needs_bootstrap(self):
        """Lanes that are non-empty, not closed, not awaiting an outcome, and whose last counted step has done == 0 and is not truncated: their last segment bootstraps
        from slot lengths[e]."""
        return np.nonzero((self.lengths > 0) & (self.state != self.CLOSED) & (self.state != self.AWAITING) & ~self._last_done())[0]

    def check_update(self):
        waiting = np.nonzero(self.state == self.AWAITING)[0]
        if waiting.size:
            raise ValueError("RolloutBuffer: update with open rows (environments %s): their last step has no outcome yet" % waiting.tolist())
        need = self.needs_bootstrap()
        if need.size:
            raise ValueError("RolloutBuffer: update with open rows (environments %s): bootstrap them first" % need.tolist())
        if int(self.lengths.sum()) < 1:
            raise ValueError("RolloutBuffer: update with no samples")

    def segments(self):
        """int32 [n_seg, 3] of (environment, first slot, length): lanes in environment order, segments in slot order; every recorded step is in exactly one."""
        out = []
        for e in range(self.num_envs):
            n = int(self.lengths[e])
            ends = (np.nonzero((self.dones[e, :n] != 0) | self.truncs[e, :n])[0] + 1).tolist()
            if n and (not ends or ends[-1] != n):
                ends.append(n)
            first = 0
            for end in ends:
                out.append((e, first, end - first))
                first = end
        return np.asarray(out, np.int32).reshape(-1, 3)

    def segment_truncated(self):
        """int32 [n_seg], in the order of segments(): 1 where the segment's last step is truncated."""
        return self._truncated(self.segments())

    def _truncated(self, segs):
        return self.truncs[segs[:, 0], segs[:, 1] + segs[:, 2] - 1].astype(np.int32)


def _real(x):
    return not isinstance(x, (bool, str)) and isinstance(x, (int, float, np.integer, np.floating))


def _finite_scalar(who, k, x, nonneg):
    """A checkpointed state's scalar `k` -> float: finite, and >= 0 with `nonneg`."""
    if not _real(x) or not np.isfinite(x) or (nonneg and x < 0):
        raise ValueError("%s: %s is a finite float%s, got %r" % (who, k, " >= 0" if nonneg else "", x))
    return float(x)


def _finite_vector(who, k, x, n, per, nonneg):
    """A checkpointed state's vector `k` -> float64 [n]: one finite number per `per`, and >= 0 with `nonneg`."""
    v = np.asarray(x)
    if v.dtype.kind not in "fiu" or v.shape != (int(n),):
        raise ValueError("%s: %s must hold one number per %s, shape (%d,), got %s %s" % (who, k, per, n, v.dtype, v.shape))
    v = v.astype(np.float64)
    if not np.isfinite(v).all() or (nonneg and (v < 0).any()):
        raise ValueError("%s: %s holds a value that is not finite%s" % (who, k, " or is negative" if nonneg else ""))
    return v


def reward_scaling_settings(clip=10.0, epsilon=1e-8, frozen=False, who="RolloutBuffer.set_reward_scaling"):
    """The checked settings of running-return reward scaling (mi_rollout_scale_rewards) -> {"clip": float, "epsilon": float, "frozen": bool}.  clip: a positive float
    (inf: never clamp); epsilon: a finite float >= 0; frozen: a bool.  Anything else raises ValueError.  numpy only: no device and no library involved."""
    if not _real(clip) or not clip > 0:
        raise ValueError("%s: clip is a positive float (inf: never clamp), got %r" % (who, clip))
    if not _real(epsilon) or not np.isfinite(epsilon) or epsilon < 0:
        raise ValueError("%s: epsilon is a finite float >= 0, got %r" % (who, epsilon))
    if not isinstance(frozen, (bool, np.bool_)):
        raise ValueError("%s: frozen is a bool, got %r" % (who, frozen))
    return {"clip": float(clip), "epsilon": float(epsilon), "frozen": bool(frozen)}


def reward_scaling_state_checked(d, num_envs, who="RolloutBuffer.load_reward_scaling_state"):
    """The checked dict of reward_scaling_state() for a buffer of num_envs lanes -> {"count", "mean", "m2": float, "carry": float64 [num_envs], and the settings}.
    count and m2 are finite and >= 0, mean and every carry finite, carry has one entry per lane.  ValueError otherwise.  numpy only."""
    keys = ("count", "mean", "m2", "carry", "clip", "epsilon", "frozen")
    if not isinstance(d, dict) or any(k not in d for k in keys):
        raise ValueError("%s: expected a dict with the keys %s" % (who, ", ".join(keys)))
    out = reward_scaling_settings(d["clip"], d["epsilon"], d["frozen"], who)
    for k in ("count", "mean", "m2"):
        out[k] = _finite_scalar(who, k, d[k], k != "mean")
    out["carry"] = _finite_vector(who, "carry", d["carry"], num_envs, "environment", False)
    return out


def minibatch_normalization_ddof(ddof=0, who="RolloutBuffer.set_minibatch_normalization"):
    """The checked delta degrees of freedom of per-minibatch advantage normalisation (mi_ppo_minibatch_advantages) -> int: 0 (population std, the project's) or 1
    (sample std, torch's .std()).  bool, str, float and every other value raise ValueError.  numpy only: no device and no library involved."""
    if isinstance(ddof, (bool, np.bool_)) or not isinstance(ddof, (int, np.integer)) or int(ddof) not in (0, 1):
        raise ValueError("%s: ddof is 0 (population std) or 1 (sample std, torch's .std()), got %r" % (who, ddof))
    return int(ddof)


def vtrace_settings(rho_bar=1.0, c_bar=1.0, who="RolloutBuffer.set_vtrace"):
    """The checked bars of V-trace (mi_rollout_finish_vtrace) -> {"rho_bar": float, "c_bar": float}.  rho_bar: a float > 0, c_bar: a float >= 0; +inf is a valid
    bar (it never truncates).  bool, str, NaN and every other value raise ValueError.  numpy only: no device and no library involved."""
    def real(x):
        return not isinstance(x, (bool, np.bool_, str)) and isinstance(x, (numbers.Real, np.floating, np.integer))
    if not real(rho_bar) or not float(rho_bar) > 0.0:
        raise ValueError("%s: rho_bar is a float > 0 (inf: the TD errors' weights are never truncated), got %r" % (who, rho_bar))
    if not real(c_bar) or not float(c_bar) >= 0.0:
        raise ValueError("%s: c_bar is a float >= 0 (inf: the trace's weights are never truncated), got %r" % (who, c_bar))
    return {"rho_bar": float(rho_bar), "c_bar": float(c_bar)}


def observation_normalization_settings(clip=10.0, epsilon=1e-8, frozen=False, normalize_latents=True, who="RolloutBuffer.set_observation_normalization"):
    """The checked settings of running observation normalisation (mi_rollout_step_batch_norm / mi_rollout_obs_stats) -> {"clip": float, "epsilon": float, "frozen":
    bool, "normalize_latents": bool}.  clip: a positive float (inf: never clamp); epsilon: a finite float >= 0; frozen, normalize_latents: bools.  Anything else raises
    ValueError.  numpy only: no device and no library involved."""
    out = reward_scaling_settings(clip, epsilon, frozen, who)
    if not isinstance(normalize_latents, (bool, np.bool_)):
        raise ValueError("%s: normalize_latents is a bool, got %r" % (who, normalize_latents))
    out["normalize_latents"] = bool(normalize_latents)
    return out


def observation_normalization_state_checked(d, din, who="RolloutBuffer.load_observation_normalization_state"):
    """The checked dict of observation_normalization_state() for observations of din columns -> {"count": float, "mean", "m2": float64 [din], "z_dim": int, and the
    settings}.  count is finite and >= 0, every mean finite, every m2 finite and >= 0, 0 <= z_dim <= din.  ValueError otherwise.  numpy only."""
    keys = ("count", "mean", "m2", "z_dim", "clip", "epsilon", "frozen", "normalize_latents")
    if not isinstance(d, dict) or any(k not in d for k in keys):
        raise ValueError("%s: expected a dict with the keys %s" % (who, ", ".join(keys)))
    out = observation_normalization_settings(d["clip"], d["epsilon"], d["frozen"], d["normalize_latents"], who)
    out["count"] = _finite_scalar(who, "count", d["count"], True)
    z_dim = d["z_dim"]
    if isinstance(z_dim, (bool, np.bool_)) or not isinstance(z_dim, (int, np.integer)) or not 0 <= int(z_dim) <= int(din):
        raise ValueError("%s: z_dim is an int in [0, %d], got %r" % (who, din, z_dim))
    out["z_dim"] = int(z_dim)
    for k in ("mean", "m2"):
        out[k] = _finite_vector(who, k, d[k], din, "observation column", k == "m2")
    return out


def _obs_norm_settings_of(d, z_dim, who, what):
    """The settings in a checked observation_normalization_state() dict, for a step or a buffer (`what`) whose latents have z_dim columns: ValueError on another z_dim."""
    if d["z_dim"] != z_dim:
        raise ValueError("%s: the state was taken with z_dim = %d, this %s has %d" % (who, d["z_dim"], what, z_dim))
    return {k: d[k] for k in ("clip", "epsilon", "frozen", "normalize_latents")}


def observation_normalization_fp32(d):
    """What the device derives from a checked state: (mean32, inv32), float32 [din] -- float32(mean) and float32(1 / sqrt(M2 / count + epsilon)) (count 0: the variance
    is 1.0), and 0 / 1 for the first z_dim columns with normalize_latents False."""
    var = d["m2"] / d["count"] if d["count"] > 0 else np.ones_like(d["m2"])
    mean32, inv32 = d["mean"].astype(np.float32), (1.0 / np.sqrt(var + np.float64(d["epsilon"]))).astype(np.float32)
    if not d["normalize_latents"]:
        mean32[:d["z_dim"]], inv32[:d["z_dim"]] = 0.0, 1.0
    return mean32, inv32


def normalize_observations(states, state_dict):
    """The formula of the normalise kernel in numpy float32, for states [..., din] and an observation_normalization_state() dict: clamp((s - mean32) * inv32, -clip,
    +clip) with one subtract and one multiply.  What a policy trained behind set_observation_normalization() must be fed by a caller that runs PPO.predict() on host
    states; also the reference of the tests.  -> float32, the shape of `states`."""
    s = np.asarray(states, np.float32)
    d = observation_normalization_state_checked(state_dict, s.shape[-1] if s.ndim else 0, "normalize_observations")
    mean32, inv32 = observation_normalization_fp32(d)
    clip = np.float32(d["clip"])
    return np.minimum(np.maximum((s - mean32) * inv32, -clip), clip)


def _obs_norm_tensors(device, din, num_envs):
    """The device side of the setting, fresh: state fp64 {count, mean[din], M2[din]}, the fp32 pair the step reads, the step's n x din buffer, the batch figures."""
    import torch
    return {"state": torch.zeros(1 + 2 * din, dtype=torch.float64, device=device), "mean32": torch.zeros(din, device=device), "inv32": torch.ones(din, device=device),
            "nstate": torch.empty(num_envs, din, device=device), "batch": torch.zeros(3, din, dtype=torch.float64, device=device)}


def _obs_norm_derive(L, on, z_dim):
    """mean32 / inv32 from the statistics as they are (mi_rollout_obs_stats with an empty list: one launch)."""
    import torch
    din = int(on["mean32"].shape[0])
    L.mi_rollout_obs_stats(torch.cuda.current_stream(on["state"].device).cuda_stream, None, 0, None, 0, din, 0 if on["normalize_latents"] else z_dim, 0, on["epsilon"],
                           on["clip"], on["state"].data_ptr(), on["mean32"].data_ptr(), on["inv32"].data_ptr(), None, on["batch"].data_ptr())


def _obs_norm_load(L, on, d, z_dim):
    import torch
    on["state"].copy_(torch.from_numpy(np.concatenate([[d["count"]], d["mean"], d["m2"]])))
    _obs_norm_derive(L, on, z_dim)


def _obs_norm_rms(on):
    state = on["state"].cpu().numpy()
    din = (state.shape[0] - 1) // 2
    count = float(state[0])
    return {"count": count, "mean": state[1:1 + din].copy(), "var": state[1 + din:] / count if count > 0 else np.ones(din)}


def _diagnostics(who, target_kl):
    """The checked arguments of update_with_diagnostics (raises before any device work): target_kl is None or a positive finite float."""
    if target_kl is not None:
        if not _real(target_kl) or not np.isfinite(target_kl) or not target_kl > 0:
            raise ValueError("%s.update_with_diagnostics: target_kl is None or a positive finite float, got %r" % (who, target_kl))
        target_kl = float(target_kl)
    return {"target_kl": target_kl}


class _StageClock:
    """The `stage_times` of an update: lap(name) closes the stage the update's chain is in and opens the next, `with stage(name)` times a stage of its own or one inside a
    chain stage; a stage ends, and one under `with` also starts, once the device is idle.  With times = None nothing is recorded and the device is never waited for."""

    def __init__(self, times, device):
        self.times, self.device, self.t = times, device, time.perf_counter()

    def _now(self):
        if self.times is not None:
            import torch
            torch.cuda.synchronize(self.device)
        return time.perf_counter()

    def _add(self, name, t0):
        if self.times is not None:
            self.times[name] = self.times.get(name, 0.0) + self._now() - t0

    def lap(self, name):
        self._add(name, self.t)
        self.t = time.perf_counter()

    @contextlib.contextmanager
    def stage(self, name):
        t0 = self._now()
        yield
        self._add(name, t0)


class _RecordingStep(BatchedRolloutStep):
    """The step of a RolloutBuffer: BatchedRolloutStep with room for the int32 table rows in its input buffer, called through check() and record(.., table_rows, tables)."""

    _who = "RolloutBuffer"
    _row_ints = 1


class RolloutBuffer:
    """Device-resident rollout buffer for `num_envs` environments and a horizon of T steps that PPO updates train from (see the module docstring).  Device tables of
    num_envs (T + 1) rows, row e (T + 1) + t = slot t of environment e: states fp32 [input_dim], actions fp32 [A], values, returns, advantages, logp_old fp32 scalars.
    Rewards and dones stay host arrays [num_envs, T] (self.rows) and are uploaded once per update."""

    _rows_class = RolloutRows

    def __init__(self, vae, ppo, num_envs, horizon, seed=None, io=None):
        self._init(vae, ppo, num_envs, horizon, seed, io, 1)

    @classmethod
    def stacked(cls, vae, ppo, num_envs, horizon, latent_stack, seed=None, io=None):
        """The buffer with LATENT STACKING (see the module docstring): cls(vae, ppo, num_envs, horizon, seed, io) whose step is BatchedRolloutStep.stacked(..,
        latent_stack): the tables' states are [z_t | the latent_stack - 1 latents before it | measurements].  ValueError before anything touches a device."""
        self = cls.__new__(cls)
        self._init(vae, ppo, num_envs, horizon, seed, io, latent_stack)
        return self

    def _init(self, vae, ppo, num_envs, horizon, seed, io, latent_stack):
        import torch
        self.rows = self._rows_class(num_envs, horizon)                              # (raises before anything touches a device)
        self.vae, self.ppo = vae, ppo
        self.num_envs, self.horizon = self.rows.num_envs, self.rows.horizon
        self._step = _RecordingStep.stacked(vae, ppo, self.num_envs, latent_stack, seed=seed, io=io)
        self.io, self.device, self.L = self._step.io, self._step.device, self._step.L
        n = self.n_table_rows = self.num_envs * (self.horizon + 1)
        self.states = torch.zeros(n, int(ppo.input_dim), device=self.device)
        self.actions = torch.zeros(n, int(ppo.num_actions), device=self.device)
        self.values, self.returns, self.advantages, self.logp_old = (torch.zeros(n, device=self.device) for _ in range(4))
        self._reward_scaling = None                                                  # running-return reward scaling (set_reward_scaling): None = off
        self._minibatch_norm = None                                                  # per-minibatch advantage normalisation (set_minibatch_normalization): None = off
        self._minibatch_advantages = None                                            # its fp32 table, allocated by the first update that needs it
        self._values_new = None                                                      # V per table row under the current parameters, allocated by the first statistics pass with value clipping on
        self._obs_norm = None                                                        # running observation normalisation (set_observation_normalization): None = off
        self.raw_states = None                                                       # its fp32 table of the raw rows, allocated when the setting is turned on
        self.mean_old = None                                                         # the old policy's action means per table row, allocated by the first update with the KL penalty on (PPO.set_kl_penalty)
        self._demo = None                                                            # the demonstration term (set_demonstrations): None = off
        self._adv_recompute = False                                                  # advantage recomputation before every later epoch (set_advantage_recomputation)
        self.values_now = None                                                       # its fp32 table: V per table row under the current parameters, allocated by the first update that needs it
        self._vtrace = None                                                          # V-trace correction of the refreshes (set_vtrace): None = off
        self.logp_now = None                                                         # its fp32 table: log pi_theta per table row under the current parameters, allocated likewise

    def set_observation_normalization(self, clip=10.0, epsilon=1e-8, frozen=False, normalize_latents=True):
        """Turns running observation normalisation on (see the module docstring): step(), bootstrap() and truncate() feed the trunks clamp((s - mean) * inv_std, +-clip)
        per column of [z | measurements] (clip inf: never clamps), `states` records the normalised rows and `raw_states` the raw ones, and the last launch of every
        update() merges the collection's raw rows into the running {count, mean, M2} kept on the device.  frozen=True: the statistics are used and not updated.
        normalize_latents=False: the first z_dim columns get mean 0 / inv_std 1 (their moments are still tracked, the clamp still applies).  Turning it on allocates the
        statistics (count 0: mean 0, inv_std 1.0) and `raw_states`; calling it again with the setting on changes the settings and keeps both.
        set_observation_normalization(None) turns it off and drops them.  Only with no step recorded (after reset()): a collection is normalised by ONE set of statistics
        and its tables hold one kind of row.  ValueError before anything touches a device."""
        settings = None if clip is None else observation_normalization_settings(clip, epsilon, frozen, normalize_latents)
        self._obs_norm_between_collections("set_observation_normalization")
        if settings is None:
            self._obs_norm = self.raw_states = self._step._obs_norm = None
            return
        _obs_norm_derive(self.L, self._obs_norm_on(settings), self._latent_cols())

    def _latent_cols(self):
        """The state's latent columns: z_dim, or latent_stack x z_dim with latent stacking on."""
        return getattr(self._step, "latent_cols", self._step.z_dim)

    def _obs_norm_between_collections(self, what):
        if (self.rows.lengths > 0).any() or self.rows.awaiting.any():
            raise ValueError("%s.%s: steps are recorded; call it after reset() -- a collection is normalised by one set of statistics" % (type(self).__name__, what))

    def _obs_norm_on(self, settings):
        import torch
        on = self._obs_norm
        if on is None:
            on = _obs_norm_tensors(self.device, int(self.states.shape[1]), self.num_envs)
            self.raw_states = torch.zeros_like(self.states)
        on.update(settings)
        self._obs_norm = self._step._obs_norm = on
        return on

    def _need_obs_norm(self, what):
        if self._obs_norm is None:
            raise ValueError("%s.%s: observation normalisation is off (set_observation_normalization)" % (type(self).__name__, what))
        return self._obs_norm

    def observation_normalization_state(self):
        """What a training script writes to its checkpoint, and what BatchedRolloutStep.set_observation_normalization() and normalize_observations() take:
        {"count": float, "mean", "m2": float64 [input_dim], "z_dim", "clip", "epsilon", "frozen", "normalize_latents"}."""
        on = self._need_obs_norm("observation_normalization_state")
        state = on["state"].cpu().numpy()
        din = int(self.states.shape[1])
        return {"count": float(state[0]), "mean": state[1:1 + din].copy(), "m2": state[1 + din:].copy(), "z_dim": self._latent_cols(), "clip": on["clip"],
                "epsilon": on["epsilon"], "frozen": on["frozen"], "normalize_latents": on["normalize_latents"]}

    def load_observation_normalization_state(self, d):
        """Takes observation_normalization_state()'s dict back: the setting is on afterwards, with these statistics and settings.  The whole dict is checked before
        anything changes (ValueError); only with no step recorded, like set_observation_normalization()."""
        d = observation_normalization_state_checked(d, int(self.states.shape[1]))
        settings = _obs_norm_settings_of(d, self._latent_cols(), type(self).__name__ + ".load_observation_normalization_state", "buffer")
        self._obs_norm_between_collections("load_observation_normalization_state")
        on = self._obs_norm_on(settings)
        _obs_norm_load(self.L, on, d, self._latent_cols())

    def merge_observation_statistics(self):
        """Merges the raw rows of the steps recorded so far (rows.valid_rows()) into the statistics NOW, without an update, and re-derives what the step reads: for a
        warm-up collection, followed by reset() -- without one the first collection runs on mean 0 / inv_std 1 and clamps a raw speed of 30 to `clip`.  The rows stay
        recorded: an update() of the same collection would merge them a second time.  ValueError with the setting off or frozen, with no step recorded, or (behind
        the launch, the statistics as they were) with a recorded observation that is not finite.
        -> update()'s `observation_rms`."""
        on = self._need_obs_norm("merge_observation_statistics")
        if on["frozen"]:
            raise ValueError("%s.merge_observation_statistics: the statistics are frozen" % type(self).__name__)
        valid = self.rows.valid_rows()
        if valid.shape[0] < 1:
            raise ValueError("%s.merge_observation_statistics: no step is recorded" % type(self).__name__)
        self._obs_norm_stats(valid, 1, "merge_observation_statistics")
        return _obs_norm_rms(on)

    def _obs_norm_stats(self, valid, merge, what):
        """One mi_rollout_obs_stats call over the table rows `valid` (host int32) -> its batch figures, float64 [3, din] on the host (batch mean, batch M2, clamped
        counts).  The device refuses to merge a batch with an entry that is not finite (one NaN would stay in mean / M2 for good, and every later step would feed the
        trunks NaN): the statistics are then as they were and this raises ValueError."""
        import torch
        on = self._obs_norm
        n, din = int(valid.shape[0]), int(self.states.shape[1])
        rows = torch.from_numpy(np.ascontiguousarray(valid, np.int32)).to(self.device)
        scratch = torch.empty(int(self.L.mi_rollout_obs_stats_scratch_doubles(n, din)), dtype=torch.float64, device=self.device)
        self.L.mi_rollout_obs_stats(torch.cuda.current_stream(self.device).cuda_stream, self.raw_states.data_ptr(), self.n_table_rows, rows.data_ptr(), n, din,
                                    0 if on["normalize_latents"] else self._latent_cols(), merge, on["epsilon"], on["clip"], on["state"].data_ptr(), on["mean32"].data_ptr(),
                                    on["inv32"].data_ptr(), scratch.data_ptr(), on["batch"].data_ptr())
        batch = on["batch"].cpu().numpy()
        if merge and not np.isfinite(batch[0]).all():
            raise ValueError("%s.%s: a recorded observation is not finite (column %d of raw_states); it would poison the statistics of observation normalisation for "
                             "good, so nothing was merged and they are as they were" % (type(self).__name__, what, int(np.flatnonzero(~np.isfinite(batch[0]))[0])))
        return batch

    def set_reward_scaling(self, clip=10.0, epsilon=1e-8, frozen=False):
        """Turns running-return reward scaling on (see the module docstring): every update divides its rewards by sqrt(var + epsilon) of the discounted returns seen so
        far, this collection included, and clamps them into +-clip (inf: never).  frozen=True: the statistics are used and not updated (the carries still advance).
        Turning it on allocates the statistics {count, mean, M2, den} and the per-lane carries on the buffer's device, all zeros; calling it again with the setting on
        changes clip / epsilon / frozen and keeps both.  set_reward_scaling(None) turns it off and drops them.  ValueError before anything touches a device."""
        if clip is None:
            self._reward_scaling = None
            return
        self._reward_scaling_on(reward_scaling_settings(clip, epsilon, frozen))

    def _reward_scaling_on(self, settings):
        import torch
        rs = self._reward_scaling
        if rs is None:
            rs = {"state": torch.zeros(4, dtype=torch.float64, device=self.device), "carry": torch.zeros(self.num_envs, dtype=torch.float64, device=self.device),
                  "scratch": torch.empty(int(self.L.mi_rollout_scale_rewards_scratch_doubles(self.num_envs)), dtype=torch.float64, device=self.device)}
        rs.update(settings)
        self._reward_scaling = rs
        return rs

    def _need_reward_scaling(self, what):
        if self._reward_scaling is None:
            raise ValueError("%s.%s: reward scaling is off (set_reward_scaling)" % (type(self).__name__, what))
        return self._reward_scaling

    def reward_scaling_state(self):
        """What a training script writes to its checkpoint: {"count", "mean", "m2": floats, "carry": float64 [num_envs], "clip", "epsilon", "frozen"}."""
        rs = self._need_reward_scaling("reward_scaling_state")
        state = rs["state"].cpu().numpy()
        return {"count": float(state[0]), "mean": float(state[1]), "m2": float(state[2]), "carry": rs["carry"].cpu().numpy(), "clip": rs["clip"],
                "epsilon": rs["epsilon"], "frozen": rs["frozen"]}

    def load_reward_scaling_state(self, d):
        """Takes reward_scaling_state()'s dict back (of this buffer or of another with as many environments): the setting is on afterwards, with these statistics, carries
        and settings.  The whole dict is checked before anything changes (ValueError)."""
        import torch
        d = reward_scaling_state_checked(d, self.num_envs)
        rs = self._reward_scaling_on({k: d[k] for k in ("clip", "epsilon", "frozen")})
        rs["state"].copy_(torch.tensor([d["count"], d["mean"], d["m2"], 0.0], dtype=torch.float64))       # (den is written by every update before it is read)
        rs["carry"].copy_(torch.from_numpy(d["carry"]))

    def zero_return_carry(self, env_ids=None):
        """The running discounted return of these environments (None: all) starts from 0.0 again: for an environment the caller reset without reporting a done or a
        truncation."""
        import torch
        rs = self._need_reward_scaling("zero_return_carry")
        if env_ids is None:
            rs["carry"].zero_()
        else:
            ids = np.asarray(env_ids)
            ids = self.rows.env_ids(ids, ids.shape[0] if ids.ndim == 1 else 0)
            rs["carry"][torch.from_numpy(ids).to(self.device)] = 0.0

    def set_advantage_recomputation(self, on=True):
        """Turns advantage recomputation on (True) or off (False / None): with it on, update() refreshes the values and with them the returns and advantages before
        every epoch but the first (see `_recompute_stage`; Andrychowicz et al. 2021).  Epoch 1 reads the values recorded at collection time, so num_epochs = 1 is bitwise the
        setting off.  `values` stays the collection-time table: value clipping reads it as V_old and the result returns it.  Needs the fused kernels (update() refuses
        otherwise).  Only with no step recorded (after reset()): with the setting on ContinuousRolloutBuffer.truncate() records the final observation's state row,
        which a collection must do for all of its truncations or for none.  ValueError before anything changes."""
        if on is not None and not isinstance(on, (bool, np.bool_)):
            raise ValueError("%s.set_advantage_recomputation: the value is True, False or None (off), got %r" % (type(self).__name__, on))
        if (self.rows.lengths > 0).any() or self.rows.awaiting.any():
            raise ValueError("%s.set_advantage_recomputation: steps are recorded; call it after reset() -- a collection records its truncations in one way" % type(self).__name__)
        self._adv_recompute = bool(on)
        if not self._adv_recompute:
            self.values_now = None

    def set_vtrace(self, rho_bar=1.0, c_bar=1.0):
        """Turns V-trace off-policy correction of the refreshes on (Espeholt et al. 2018): with advantage recomputation on, every refresh also runs ONE
        mi_ppo_logp_idx call -- log pi_theta of the recorded rows under the current parameters -- and its finish call is mi_rollout_finish_vtrace on the refreshed
        values, that table and the update's cache of log pi_old: truncated importance weights min(rho_bar, pi_theta / pi_old) on the TD errors and
        lam min(c_bar, pi_theta / pi_old) on the trace.  The first finish call stays the GAE call (theta == theta_old there: V-trace equals it), so one epoch is bitwise
        the setting off; the SGD steps still take log pi_old from the cache.  rho_bar: a float > 0, c_bar: a float >= 0 (inf: that bar never truncates).
        set_vtrace(None) turns it off and drops the table.  update() refuses V-trace without advantage recomputation.  ValueError before anything changes."""
        if rho_bar is None:
            self._vtrace = self.logp_now = None
            return
        self._vtrace = vtrace_settings(rho_bar, c_bar, type(self).__name__ + ".set_vtrace")

    def set_minibatch_normalization(self, ddof=0):
        """Turns per-minibatch advantage normalisation on (see the module docstring): in front of every epoch one mi_ppo_minibatch_advantages call normalises the raw
        advantages of each of the epoch's minibatches by that minibatch's own mean and std (ddof = 0: population std; 1: sample std, torch's .std()) into a table of its
        own, which the epoch's SGD steps read in place of `advantages`.  set_minibatch_normalization(None) turns it off and drops the table.  ValueError before anything
        touches a device."""
        if ddof is None:
            self._minibatch_norm = self._minibatch_advantages = None
            return
        self._minibatch_norm = {"ddof": minibatch_normalization_ddof(ddof)}

    def set_demonstrations(self, demo_buffer, coef=None, loss="nll", batch_size=32, decay=1.0, seed=0):
        """Turns the demonstration term on (see the module docstring): every SGD step of update() / update_with_diagnostics() is one PPO._demo_rows call on the PPO
        minibatch plus min(batch_size, demo_buffer.size) rows of `demo_buffer` (a DemonstrationBuffer of the same policy), loss = L_ppo + coef x clone_loss(those
        rows) with loss "nll" or "mse"; after every update coef *= decay.  The rows come from a np.random.RandomState(seed) of this setting's own
        (demonstration_rows_drawn: a permutation and a cursor); the legacy numpy stream is consumed as with the setting off.  set_demonstrations(None) turns it off.  ValueError before
        anything touches a device: coef not a finite float >= 0, an unknown loss, batch_size < 1, decay not a finite float >= 0, and every refusal of
        _check_demonstrations."""
        if demo_buffer is None:
            self._demo = None
            return
        who = type(self).__name__ + ".set_demonstrations"
        if not isinstance(demo_buffer, DemonstrationBuffer):
            raise ValueError("%s: demo_buffer is a DemonstrationBuffer or None, got %r" % (who, type(demo_buffer).__name__))
        for name, v in (("coef", coef), ("decay", decay)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not (v >= 0 and v < float("inf")):
                raise ValueError("%s: %s is a finite float >= 0, got %r" % (who, name, v))
        kind = milib.clone_kind(loss, who)
        for name, v in (("batch_size", batch_size), ("seed", seed)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not (1 if name == "batch_size" else 0) <= int(v) < 1 << 32:
                raise ValueError("%s: %s is an int >= %d, got %r" % (who, name, 1 if name == "batch_size" else 0, v))
        dm = {"buffer": demo_buffer, "coef": float(coef), "loss": ("nll", "mse")[kind], "batch_size": int(batch_size), "decay": float(decay),
              "rng": np.random.RandomState(int(seed)), "perm": None, "cursor": 0}
        self._check_demonstrations(dm, who)
        self._demo = dm

    def _check_demonstrations(self, dm, who):
        """What the demonstration term refuses, when it is set and again in front of every update: an empty demonstration buffer, another input_dim / action count /
        ppo object, a stacked rollout buffer, observation normalisation that does not match (off in both buffers, or frozen here and equal by value to the state
        the demonstration buffer was given) and a policy outside the fused kernels' range."""
        import torch
        db = dm["buffer"]
        if self._stacked():
            raise ValueError(who + ": latent stacking is on and DemonstrationBuffer has no stacked form")
        if db.size < 1:
            raise ValueError(who + ": the demonstration buffer is empty")
        if db.ppo is not self.ppo:
            raise ValueError(who + ": the demonstration buffer belongs to another ppo object")
        if int(db.states.shape[1]) != int(self.states.shape[1]) or int(db.A) != int(self.actions.shape[1]):
            raise ValueError("%s: the demonstration buffer's rows are [%d inputs, %d actions], this buffer's [%d, %d]"
                             % (who, db.states.shape[1], db.A, self.states.shape[1], self.actions.shape[1]))
        mine, theirs = self._obs_norm, db._step._obs_norm
        if (mine is None) != (theirs is None):
            raise ValueError(who + ": observation normalisation is on in one buffer and off in the other: the demonstration rows and the rollout rows are not the same kind of state")
        if mine is not None:
            same = all(mine[k] == theirs[k] for k in ("clip", "epsilon", "normalize_latents")) and torch.equal(mine["state"], theirs["state"])
            if not (mine["frozen"] and same):
                raise ValueError(who + ": with observation normalisation on, this buffer's statistics must be frozen and equal to the state the demonstration buffer was given "
                                 "(DemonstrationBuffer.set_observation_normalization(observation_normalization_state()))")
        self.ppo._clone_kind(who, dm["loss"])                                        # (the fused range, without a device)
        if self.ppo.dev is not None and not self.ppo.dev.fused_ok():
            raise ValueError(who + ": the demonstration term exists only in the fused kernels (this policy's shape is outside their range (more than 96 inputs: "
                             "PPO.set_wide_inputs()) or MI355_PPO_FUSED=0)")

    def _need_demonstrations(self, what):
        if getattr(self, "_demo", None) is None:
            raise ValueError("%s.%s: the demonstration term is off (set_demonstrations)" % (type(self).__name__, what))
        return self._demo

    @staticmethod
    def demonstration_rows_drawn(dm, n, steps):
        """The draw rule: `steps` minibatches of m = min(batch_size, n) rows of a demonstration buffer of n rows -> int32 [steps, m].  The setting keeps a permutation of
        the n rows and a cursor; a minibatch is the next m rows of the permutation, and when fewer than m remain (or there is no permutation of n rows yet) a fresh
        rng.permutation(n) is drawn first and the cursor returns to 0."""
        m = min(dm["batch_size"], n)
        out = np.zeros((steps, m), np.int32)
        for i in range(steps):
            if dm["perm"] is None or dm["perm"].shape[0] != n or n - dm["cursor"] < m:
                dm["perm"], dm["cursor"] = dm["rng"].permutation(n), 0
            out[i] = dm["perm"][dm["cursor"]:dm["cursor"] + m]
            dm["cursor"] += m
        return out

    def demonstration_state(self):
        """What a training script writes to its checkpoint: {"coef", "rng" (RandomState.get_state()), "perm" (int64 [n] or None), "cursor"}."""
        dm = self._need_demonstrations("demonstration_state")
        return {"coef": dm["coef"], "rng": dm["rng"].get_state(), "perm": None if dm["perm"] is None else np.array(dm["perm"], np.int64), "cursor": int(dm["cursor"])}

    def load_demonstration_state(self, d):
        """Takes demonstration_state()'s dict back (the setting must be on); the whole dict is checked before anything changes (ValueError)."""
        dm = self._need_demonstrations("load_demonstration_state")
        who = type(self).__name__ + ".load_demonstration_state"
        if not isinstance(d, dict) or set(d) != {"coef", "rng", "perm", "cursor"}:
            raise ValueError(who + ": expected the keys coef, rng, perm and cursor")
        coef, cursor = d["coef"], d["cursor"]
        if isinstance(coef, (bool, np.bool_)) or not isinstance(coef, (int, float, np.integer, np.floating)) or not (coef >= 0 and coef < float("inf")):
            raise ValueError("%s: coef is a finite float >= 0, got %r" % (who, coef))
        perm = None if d["perm"] is None else np.array(d["perm"], np.int64).reshape(-1)
        if perm is not None and not np.array_equal(np.sort(perm), np.arange(perm.shape[0])):
            raise ValueError(who + ": perm is not a permutation")
        if isinstance(cursor, (bool, np.bool_)) or not isinstance(cursor, (int, np.integer)) or not 0 <= int(cursor) <= (0 if perm is None else perm.shape[0]):
            raise ValueError("%s: cursor is an int inside the permutation, got %r" % (who, cursor))
        rng = np.random.RandomState(0)
        try:
            rng.set_state(d["rng"])
        except Exception as e:                                                       # (numpy raises TypeError, ValueError or IndexError by what is wrong with it)
            raise ValueError("%s: rng is not a RandomState state (%s)" % (who, e))
        dm["coef"], dm["rng"], dm["perm"], dm["cursor"] = float(coef), rng, perm, int(cursor)

    @property
    def lengths(self):
        return self.rows.lengths

    def reset(self):
        """All rows empty and open.  (The statistics and carries of reward scaling belong to the run, not to a collection: they stay -- and so do the latent history
        and its fresh flags: an episode may continue across an update.)"""
        self.rows.reset()

    def _stacked(self):
        return getattr(self._step, "k", 1) > 1                                       # latent stacking (latent_stack > 1)

    def _lanes(self, env_ids, n):
        """The history lanes of a call, with latent stacking on: its environments."""
        return self.rows.env_ids(env_ids, n) if self._stacked() else None

    @property
    def history(self):
        """Latent stacking: the device tensor [num_envs, latent_stack - 1, z_dim] (slot 0: the latent of the lane's previous step); None with the setting off."""
        return getattr(self._step, "history", None)                                  # (never allocated with the setting off)

    def restart_history(self, env_ids=None):
        """These environments (None: all) were reset without a done or a truncation being reported: their next step starts an episode (its row repeats its own
        latent), as zero_return_carry() does for reward scaling."""
        if env_ids is not None:
            ids = np.asarray(env_ids)
            env_ids = self.rows.env_ids(ids, ids.shape[0] if ids.ndim == 1 else 0)
        self._step.restart(env_ids)

    def history_state(self):
        """What a training script writes to its checkpoint: {"latent_stack", "z_dim", "history": float32 [num_envs, latent_stack - 1, z_dim], "fresh": bool [num_envs]}."""
        return self._step.history_state()

    def load_history_state(self, d):
        """Takes history_state()'s dict back (of this buffer or of another of the same shape).  The whole dict is checked before anything changes (ValueError)."""
        self._step.load_history_state(d)

    def step(self, frames_u8, measurements, env_ids=None, greedy=False, noise=None):
        """BatchedRolloutStep.__call__ of these frames, and row i of the call is recorded at slot lengths[env_ids[i]] of environment env_ids[i] (None: 0 .. n-1).
        With latent stacking on the environments' history advances."""
        f, n, meas, nz = self._step.check(frames_u8, measurements, greedy, noise)
        rows = self.rows.step_rows(env_ids, n)
        return self._step.record(f, n, meas, nz, greedy, rows, self.states, self.actions, self.values, self.raw_states, lanes=self._lanes(env_ids, n))

    def outcome(self, rewards, dones, env_ids=None):
        """Reward and done of the step just recorded for these environments (the simulator's answer to the action); the row's length grows by one.  With latent
        stacking on, an environment that reports done starts its next step from a fresh history."""
        self.rows.outcome(rewards, dones, env_ids)
        if self._stacked():
            d = np.asarray(dones)
            self._step.fresh[self.rows.env_ids(env_ids, d.shape[0])[d.astype(bool)]] = True

    def bootstrap(self, frames_u8, measurements, env_ids=None):
        """The state after the last step of these environments (None: every stepped row still open) and its value into slot lengths[e] (train.py:172; computed after a
        terminal too, the terminal flag masks it); closes the rows.  A greedy recording call: the action slot it writes is never read."""
        if env_ids is None:
            env_ids = self.rows.stepped()
        f, n, meas, _ = self._step.check(frames_u8, measurements, True, None)
        rows = self.rows.bootstrap_rows(env_ids, n)
        # (latent stacking: the history is read and not advanced -- the same observation is stepped again when the episode continues into the next collection)
        return self._step.record(f, n, meas, None, True, rows, self.states, self.actions, self.values, self.raw_states, lanes=self._lanes(env_ids, n), advance=False)

    def update(self, gamma=0.99, lam=0.95, num_epochs=3, batch_size=32, stage_times=None):
        """One PPO update from the tables (train.py:175-207 over the recorded rows): mi_rollout_finish, update_old_policy, log pi_old once, num_epochs x shuffled
        minibatches of batch_size (the last one partial) with the gather inside the step's kernels.  Returns the per-minibatch loss records (replay_update's keys),
        `lengths`, and fp64 `returns` / `advantages` / `raw_advantages` and fp32 `values` as [num_envs, T] arrays, NaN beyond a row's length.  With
        ppo.max_grad_norm set (PPO.set_max_grad_norm) also `grad_norms` and `clip_scales`, float32 [number of SGD steps]: each step's global gradient norm before
        clipping and the factor it was scaled by.  With reward scaling on (set_reward_scaling) mi_rollout_scale_rewards runs in front of the finish call with this
        update's gamma, the finish reads the scaled rewards, and the result gains `return_rms`, `reward_scale_den`, `scaled_rewards`, `discounted_returns`,
        `reward_clip_fraction` and `return_carry`; `stage_times` gains "reward_scaling", which is also part of "finish".  A reward that is not finite in a recorded
        step then raises ValueError before anything is launched or changed.  With per-minibatch normalisation on (set_minibatch_normalization) one
        mi_ppo_minibatch_advantages call runs in front of every epoch's first step over that epoch's shuffled rows, and the steps gather their advantage from the table
        it writes: `advantages` is still the finish call's output, but the SGD steps did NOT read it.  The result gains `minibatch_adv_stats`, float64 [number of SGD
        steps, 3] = every step's {count, mean, std} in step order, and `minibatch_advantages`, float32 [num_envs, T]: what the steps of the last epoch that ran read
        (NaN beyond a row's length, all NaN for num_epochs = 0); `stage_times` gains "minibatch_norm", which is also part of "sgd".  With observation normalisation on
        (set_observation_normalization) the last launch is mi_rollout_obs_stats over `raw_states` at rows.valid_rows() (merging unless frozen), and the result gains
        `observation_rms` = {"count", "mean" [input_dim], "var" [input_dim]} and `observation_clip_fraction`, float64 [input_dim]; `stage_times` gains
        "observation_stats".  A recorded observation that is not finite is not merged: ValueError behind that last launch, the statistics as they were.
        With advantage recomputation on (set_advantage_recomputation) every epoch but the first starts with a refresh (_recompute_stage: one mi_ppo_values_idx call
        into `values_now`, then the finish call again on it): the steps of that epoch gather the refreshed returns and advantages, the result gains
        `recomputed_epochs` and, when a refresh ran, `refreshed_values` / `refreshed_returns` / `refreshed_advantages` / `refreshed_raw_advantages` of the last one;
        `returns` / `advantages` / `raw_advantages` / `values` stay the first finish call's and the recorded ones; `stage_times` gains "recompute", which is also
        part of "sgd"."""
        return self._run_update(gamma, lam, num_epochs, batch_size, stage_times, None)

    def update_with_diagnostics(self, gamma=0.99, lam=0.95, num_epochs=3, batch_size=32, stage_times=None, target_kl=None):
        """update() that also OBSERVES every epoch: after an epoch's last minibatch one forward-only statistics pass (mi_ppo_update_stats_idx) runs over all valid rows of
        the tables `states`, `actions`, `returns`, `logp_old` in chunks of at most 4096 entries of valid_rows() (the first stores its sums, the later ones add to them),
        with one readback per epoch.  The result gains `epochs`, one dict per epoch that ran (mi355.ppo_device.update_stats_summary: samples, approx_kl -- the k3
        estimator, mean of r - 1 - log r against the old policy --, approx_kl_k1, clip_fraction, ratio_mean, value_mse, explained_variance), `epochs_run` and
        `stopped_early`; `stage_times` gains a "stats" stage.  The pass changes nothing the SGD steps read: parameters and losses are bitwise those of update() on the
        same inputs and numpy seed.
        target_kl (None, or a positive finite float): after an epoch whose approx_kl is greater than target_kl -- a plain `>`; other libraries stop at 1.5 x their
        target_kl, so pass 1.5 x theirs to compare -- no further epoch runs and `stopped_early` is True.  np.random.shuffle is then called once per epoch that RAN, so
        the legacy numpy stream is left where an update of `epochs_run` epochs leaves it.
        With ppo.max_grad_norm set, every dict of `epochs` also holds `grad_norm_max` (the largest norm among the epoch's steps) and `clipped_steps` (how many of them
        were scaled down), from the same arrays as `grad_norms` / `clip_scales`: no further readback.
        With ppo.value_clip set (PPO.set_value_clip), every dict of `epochs` also holds `value_clip_fraction`, `value_loss_clipped` and `value_grad_zero_fraction`
        (mi355.ppo_device.value_clip_summary): the statistics pass also writes V per table row, mi_ppo_value_clip_stats runs over the same chunks, and both sets of
        sums come back in the epoch's one readback.
        With ppo.dual_clip set (PPO.set_dual_clip), every dict of `epochs` also holds `dual_clip_fraction`, `negative_advantage_fraction`, `surrogate_mean` and
        `surrogate_mean_unclipped` (mi355.ppo_device.dual_clip_summary): the statistics pass also writes log pi_theta per table row, mi_ppo_dual_clip_stats runs over
        the same chunks on it, the cached log pi_old and the advantage table the epoch's steps gathered from, and its sums come back in the same readback.
        With reward scaling on (set_reward_scaling) the returns table holds returns of the SCALED rewards: value_mse and explained_variance are measured on those.
        With advantage recomputation on (set_advantage_recomputation) the returns table holds, from epoch 2 on, the REFRESHED returns of that epoch: value_mse and
        explained_variance are measured against those.
        Needs the cached log pi_old, i.e. the fused kernels (PpoDevice.fused_ok()): ValueError otherwise, before anything is launched or changed."""
        return self._run_update(gamma, lam, num_epochs, batch_size, stage_times, _diagnostics(type(self).__name__, target_kl))

    def _run_update(self, gamma, lam, num_epochs, batch_size, stage_times, diag):
        def finish(st, r, d, lengths, f64, now=False, vt=None):
            import torch
            if vt is not None:                                                       # a V-trace refresh: one segment per non-empty lane (slot 0, its length), mi_rollout_finish's successor rule
                lanes = np.nonzero(lengths > 0)[0]
                desc = torch.from_numpy(np.stack([lanes * (self.horizon + 1), np.minimum(lengths[lanes], self.horizon)]).astype(np.int32)).to(self.device)
                self.L.mi_rollout_finish_vtrace(st, self.values_now.data_ptr(), vt["logp_now"].data_ptr(), vt["logp_old"].data_ptr(), r.data_ptr(), d.data_ptr(), desc[0].data_ptr(),
                                                desc[1].data_ptr(), int(lanes.shape[0]), self.num_envs, self.horizon, float(gamma), float(lam), vt["rho_bar"], vt["c_bar"], 1, 0,
                                                None, self.returns.data_ptr(), self.advantages.data_ptr(), f64[0].data_ptr(), f64[1].data_ptr(), f64[2].data_ptr(),
                                                vt["weights"].data_ptr(), None, None)
                return
            ln = torch.from_numpy(lengths).to(self.device)
            self.L.mi_rollout_finish(st, (self.values_now if now else self.values).data_ptr(), r.data_ptr(), d.data_ptr(), ln.data_ptr(), self.num_envs, self.horizon, float(gamma), float(lam),
                                     self.returns.data_ptr(), self.advantages.data_ptr(), f64[0].data_ptr(), f64[1].data_ptr(), f64[2].data_ptr())
        return self._update(finish, num_epochs, batch_size, stage_times, diag, gamma)

    def _update(self, finish, num_epochs, batch_size, stage_times, diag=None, gamma=None, truncs=None):
        """What every buffer's update does around its finish call `finish(stream, rewards, dones, lengths, f64, now=False)` (device rewards / dones, fp64 [3, E, T] of NaN for
        the raw advantages, returns and normalised advantages; now=True: the call reads the refreshed value tables instead of the recorded ones): check, upload,
        scale the rewards, finish, cache log pi_old, the epochs, the result, the observation statistics.
        A stage of an optional setting runs only with that setting on.  diag: None, or update_with_diagnostics' {"target_kl": None or float}.  gamma, truncs (host bool
        [E, T] or None): what the reward scaling pass in front of the finish call takes, read only with the setting on."""
        import torch
        vclip = getattr(self.ppo, "value_clip", None)                                # PPO2-style value clipping (PPO.set_value_clip): None = off
        klp = getattr(self.ppo, "kl_penalty", None)                                  # adaptive KL penalty (PPO.set_kl_penalty): None = off
        recorded = self._check_update(num_epochs, batch_size, vclip, diag, klp)
        rs = self._reward_scaling                                                    # running-return reward scaling (set_reward_scaling): None = off
        mbn = getattr(self, "_minibatch_norm", None)                                 # per-minibatch advantage normalisation (set_minibatch_normalization): None = off
        on = getattr(self, "_obs_norm", None)                                        # running observation normalisation (set_observation_normalization): None = off
        demo = getattr(self, "_demo", None)                                          # the demonstration term (set_demonstrations): None = off
        E, T, device = self.num_envs, self.horizon, self.device
        valid = self.rows.valid_rows()
        # this update: what its stages share, and what they leave for the result
        u = types.SimpleNamespace(batch_size=int(batch_size), num_epochs=int(num_epochs), vclip=vclip, klp=klp, diag=diag, mbn=mbn, demo=demo, valid=valid, n_valid=int(valid.shape[0]),
                                  lengths=self.rows.lengths.copy(), recorded=recorded, clock=_StageClock(stage_times, device),
                                  st=torch.cuda.current_stream(device).cuda_stream)
        r = torch.from_numpy(self.rows.rewards).to(device)
        d = torch.from_numpy(self.rows.dones).to(device)
        u.f64 = torch.full((3, E, T), float("nan"), dtype=torch.float64, device=device)    # raw advantages, returns, normalised advantages (inspection)
        u.f64_cur = u.f64                                                            # the triple of the epoch that runs: a refresh puts its own in its place
        if rs is not None:
            scaled = self._scale_rewards(u, rs, r, d, gamma, truncs)
            r = scaled[1]                                                            # what the finish call reads
        finish(u.st, r, d, u.lengths, u.f64)
        u.clock.lap("finish")
        u.recompute = self._recompute_stage(u, finish, r, d) if getattr(self, "_adv_recompute", False) else None
        self.ppo.update_old_policy()
        logp_old = self._cache_logp_old(valid, klp is not None)
        u.logp_old = logp_old                                                        # (a V-trace refresh reads the cache as well: its closure was made in front of this stage)
        u.clock.lap("logp_old")
        self._run_epochs(u, logp_old)
        out = self._result(u)
        if u.recompute is not None:
            self._recompute_result(u, out)
        if klp is not None:
            self._kl_penalty_result(u, out)
        if mbn is not None:
            self._minibatch_norm_result(u, out)
        if demo is not None:
            self._demonstration_result(u, out)
        if rs is not None:
            self._reward_scaling_result(u, rs, scaled, out)
        if on is not None:                                                           # the update's last launch: nothing above can raise behind it
            self._observation_stats(u, on, out)
        return out

    def _check_update(self, num_epochs, batch_size, vclip, diag, klp=None):
        """Every refusal of an update, before anything is launched or changed -> the slots that hold a recorded step, bool [num_envs, horizon]."""
        from mi355 import dist as midist
        who = type(self).__name__
        if midist.world_size() > 1:
            raise ValueError(who + ".update: single rank only (ragged rows give ranks different numbers of gradient all-reduces)")
        if int(batch_size) < 1 or int(num_epochs) < 0:
            raise ValueError(who + ".update: batch_size >= 1, num_epochs >= 0")
        if vclip is not None and not self.ppo._need_dev().fused_ok():
            raise ValueError(who + ".update: value clipping (PPO.set_value_clip) exists only in the fused kernels (this policy's shape is outside their range (more than 96 inputs: PPO.set_wide_inputs()) or "
                             "MI355_PPO_FUSED=0)")
        if klp is not None and not self.ppo._need_dev().fused_ok():
            raise ValueError(who + ".update: the KL penalty (PPO.set_kl_penalty) exists only in the fused kernels (this policy's shape is outside their range (more than 96 inputs: PPO.set_wide_inputs()) or "
                             "MI355_PPO_FUSED=0)")
        if getattr(self.ppo, "dual_clip", None) is not None and not self.ppo._need_dev().fused_ok():
            raise ValueError(who + ".update: dual clip (PPO.set_dual_clip) exists only in the fused kernels (this policy's shape is outside the fused range (more than 96 inputs: PPO.set_wide_inputs()) or "
                             "MI355_PPO_FUSED=0)")
        if getattr(self, "_adv_recompute", False) and not self.ppo._need_dev().fused_ok():
            raise ValueError(who + ".update: advantage recomputation (set_advantage_recomputation) exists only in the fused kernels (this policy's shape is outside the fused range (more than 96 inputs: PPO.set_wide_inputs()) or "
                             "MI355_PPO_FUSED=0)")
        if getattr(self, "_vtrace", None) is not None:
            if not getattr(self, "_adv_recompute", False):
                raise ValueError(who + ".update: V-trace (set_vtrace) corrects the refreshes of advantage recomputation, which is off (set_advantage_recomputation)")
            if not self.ppo._need_dev().fused_ok():
                raise ValueError(who + ".update: V-trace (set_vtrace) exists only in the fused kernels (this policy's shape is outside the fused range (more than 96 inputs: PPO.set_wide_inputs()) or "
                                 "MI355_PPO_FUSED=0)")
        if diag is not None and not self.ppo._need_dev().fused_ok():
            raise ValueError(who + ".update_with_diagnostics: the statistics pass reads the cached log pi_old, which only the fused kernels fill "
                             "(this policy's shape is outside their range (more than 96 inputs: PPO.set_wide_inputs()) or MI355_PPO_FUSED=0)")
        if getattr(self, "_demo", None) is not None:
            self._check_demonstrations(self._demo, who + ".update")
        self.rows.check_update()
        recorded = np.arange(self.horizon)[None, :] < self.rows.lengths[:, None]
        if self._reward_scaling is not None and not np.isfinite(self.rows.rewards[recorded]).all():
            raise ValueError(who + ".update: a recorded reward is not finite; it would poison the statistics of reward scaling for good")
        return recorded

    def _recompute_rows(self, u):
        """The table rows a refresh values: every recorded step and the bootstrap slot lengths[e] of every non-empty lane (int32, host)."""
        lanes = np.nonzero(u.lengths > 0)[0]
        return np.concatenate([u.valid, (self.rows._base[lanes] + u.lengths[lanes]).astype(np.int32)]).astype(np.int32)

    def _recompute_extra(self, u):
        """What a refresh does between its value pass and its finish call (ContinuousRolloutBuffer: the final observations of the truncated steps)."""

    def _recompute_stage(self, u, finish, r, d):
        """Advantage recomputation (set_advantage_recomputation) -> refresh(), which _run_epochs calls before every epoch but the first (stage "recompute", also part
        of "sgd"; a KL stop ends the refreshes with the epochs).  A refresh is ONE mi_ppo_values_idx call -- the value net alone under the current parameters -- over
        _recompute_rows() of `states` into `values_now`, and the update's finish call again with `values_now` in the place of `values`: the same rewards (scaled, with
        reward scaling on), dones, lengths or segments, gamma, lam and normalisation.  It rewrites `returns` and `advantages`, which the steps gather from, and a second
        fp64 triple, which per-minibatch normalisation then reads.  `values_now` starts every update as a copy of `values`; `values` is never written."""
        import torch
        pdev, device = self.ppo._need_dev(), self.device
        if getattr(self, "values_now", None) is None:
            self.values_now = torch.zeros(self.n_table_rows, device=device)
        self.values_now.copy_(self.values)
        rows = torch.from_numpy(self._recompute_rows(u)).to(device)
        u.f64_now = torch.full((3, self.num_envs, self.horizon), float("nan"), dtype=torch.float64, device=device)
        u.recomputed = 0

        vtrace = getattr(self, "_vtrace", None)                                      # V-trace off-policy correction of the refreshes (set_vtrace): None = off
        if vtrace is not None:
            # log pi_theta of the recorded rows under the current parameters, and the weights exp(log pi_theta - log pi_old) the last refresh formed.  The cache
            # of log pi_old is filled behind this stage: refresh() takes it from u.logp_old
            valid_dev = torch.from_numpy(u.valid).to(device)
            if getattr(self, "logp_now", None) is None:
                self.logp_now = torch.zeros(self.n_table_rows, device=device)
            u.vt_weights = torch.full((self.num_envs, self.horizon), float("nan"), dtype=torch.float64, device=device)

        def refresh():
            with u.clock.stage("recompute"):
                pdev.values_idx(self.states, rows, int(rows.numel()), self.values_now)
                if vtrace is None:
                    self._recompute_extra(u)
                    finish(u.st, r, d, u.lengths, u.f64_now, now=True)
                else:
                    pdev.logp_idx(self.states, self.actions, valid_dev, int(valid_dev.numel()), self.logp_now)
                    self._recompute_extra(u)
                    finish(u.st, r, d, u.lengths, u.f64_now, now=True, vt={"rho_bar": vtrace["rho_bar"], "c_bar": vtrace["c_bar"], "logp_now": self.logp_now,
                                                                           "logp_old": u.logp_old, "weights": u.vt_weights})
                u.f64_cur = u.f64_now
                u.recomputed += 1
        return refresh

    def _recompute_result(self, u, out):
        out["recomputed_epochs"] = int(u.recomputed)
        if not u.recomputed:
            return
        E, T = self.num_envs, self.horizon
        f64 = u.f64_now.cpu().numpy()
        out["refreshed_raw_advantages"], out["refreshed_returns"], out["refreshed_advantages"] = f64[0], f64[1], f64[2]
        out["refreshed_values"] = np.where(u.recorded, self.values_now.view(E, T + 1)[:, :T].cpu().numpy(), np.float32(np.nan)).astype(np.float32)
        vtrace = getattr(self, "_vtrace", None)
        if vtrace is not None:                                                       # the last refresh's importance weights, and how many of them each bar truncated
            w = u.vt_weights.cpu().numpy()
            out["refreshed_importance_weights"] = w
            out["vtrace_rho_clip_fraction"] = float((w[u.recorded] > vtrace["rho_bar"]).mean())
            out["vtrace_c_clip_fraction"] = float((w[u.recorded] > vtrace["c_bar"]).mean())

    def _scale_rewards(self, u, rs, r, d, gamma, truncs):
        """The reward-scaling pass in front of the finish call (mi_rollout_scale_rewards) -> fp64 [2, E, T] on the device: discounted returns G, scaled rewards."""
        import torch
        E, T, device = self.num_envs, self.horizon, self.device
        with u.clock.stage("reward_scaling"):
            scaled = torch.full((2, E, T), float("nan"), dtype=torch.float64, device=device)
            tr = None if truncs is None else torch.from_numpy(truncs.astype(np.uint8)).to(device)
            ln = torch.from_numpy(np.ascontiguousarray(u.lengths, np.int32)).to(device)
            self.L.mi_rollout_scale_rewards(u.st, r.data_ptr(), d.data_ptr(), milib.ptr(tr), ln.data_ptr(), E, T, float(gamma), rs["epsilon"], rs["clip"],
                                            0 if rs["frozen"] else 1, rs["state"].data_ptr(), rs["carry"].data_ptr(), rs["scratch"].data_ptr(), scaled[0].data_ptr(),
                                            scaled[1].data_ptr())
        return scaled

    def _reward_scaling_result(self, u, rs, scaled, out):
        state, scaled = rs["state"].cpu().numpy(), scaled.cpu().numpy()
        out["return_rms"] = {"count": float(state[0]), "mean": float(state[1]), "var": float(state[2] / state[0]) if state[0] > 0 else 1.0}
        out["reward_scale_den"] = float(state[3])
        out["discounted_returns"], out["scaled_rewards"] = scaled[0], scaled[1]
        out["reward_clip_fraction"] = float((np.abs(scaled[1][u.recorded]) == rs["clip"]).mean())
        out["return_carry"] = rs["carry"].cpu().numpy()

    def _cache_logp_old(self, valid, with_means=False):
        """theta_old is fixed for the whole update: log pi_old(a | s) once per table row, in chunks of 4096 rows that hold a recorded step (slots that hold none are
        computed along and never read: the tables start as zeros).  -> the table, or None without the fused kernels.  with_means (the KL penalty is on): the same
        pass also fills the table `mean_old` [n_table_rows, A] with the old policy's action means (mi_ppo_old_policy_cache)."""
        pdev = self.ppo._need_dev()
        if not pdev.fused_ok():
            return None
        if with_means and self.mean_old is None:
            import torch
            self.mean_old = torch.zeros(self.n_table_rows, int(self.ppo.num_actions), device=self.device)
        for lo in range(0, self.n_table_rows, 4096):
            hi = min(lo + 4096, self.n_table_rows)
            if np.any((valid >= lo) & (valid < hi)):
                if with_means:
                    pdev.old_policy_cache(self.states[lo:hi], self.actions[lo:hi], hi - lo, self.logp_old[lo:hi], self.mean_old[lo:hi])
                else:
                    pdev.logp_old(self.states[lo:hi], self.actions[lo:hi], hi - lo, self.logp_old[lo:hi])
        return self.logp_old

    def _run_epochs(self, u, logp_old):
        """The epochs of shuffled minibatches.  Leaves in `u`: records (every step's losses), clips (with gradient clipping on, every step's {norm, scale, c, 0}), with
        diagnostics epochs (a dict per epoch that ran), epoch_first (the index into clips of every epoch's first step) and stopped (the KL stop), and with per-minibatch
        normalisation mb_stats ({count, mean, std} of every step) and mb_epochs (how many epochs it holds)."""
        import torch
        ppo, pdev, device, n_valid, batch_size = self.ppo, self.ppo._need_dev(), self.device, u.n_valid, u.batch_size
        step_kw = {} if u.vclip is None else {"old_values_all": self.values}         # the values recorded at collection time: the table the finish call read
        if u.klp is not None:                                                        # the KL penalty: every step's [mean KL, penalty] is kept as well
            u.kl_coef, u.kl_records = ppo.kl_penalty, []
        clip = ppo.max_grad_norm is not None                                         # global-norm clipping on: every step's {norm, scale, c, 0} is kept as well
        records, clips = [], []
        u.records, u.clips, u.epoch_first, u.epochs, u.stopped, u.mb_epochs = records, clips, [0], [], False, 0
        if u.demo is not None:                                                       # the demonstration term: this update's coefficient and loss go to every step; the policy's own setting is not touched
            db = u.demo["buffer"]
            u.demo_coef, u.demo_records, u.demo_rows = u.demo["coef"], [], []
            steps_per_epoch, md = -(-n_valid // batch_size), min(u.demo["batch_size"], db.size)
        adv_table = self.advantages                                                  # the table the steps gather their advantage from
        if u.mbn is not None:
            if getattr(self, "_minibatch_advantages", None) is None:
                self._minibatch_advantages = torch.zeros(self.n_table_rows, device=device)
            adv_table = self._minibatch_advantages
            u.mb_stats = torch.zeros(u.num_epochs, -(-n_valid // batch_size), 3, dtype=torch.float64, device=device)
        u.adv_table = adv_table                                                      # (the dual-clip diagnostics read the advantages the steps read)
        observe = self._stats_pass(u) if u.diag is not None else None
        for epoch in range(u.num_epochs):
            if u.recompute is not None and epoch > 0:                                # every later epoch that runs: values, returns and advantages under the current parameters
                u.recompute()
            indices = np.arange(n_valid)
            np.random.shuffle(indices)                                               # legacy numpy RNG, as train.py:194-195
            perm = torch.from_numpy(u.valid[indices]).to(device)                     # shuffled positions -> table rows
            if u.mbn is not None:                                                    # this epoch's minibatches, each normalised alone, from the raw advantages
                with u.clock.stage("minibatch_norm"):
                    self.L.mi_ppo_minibatch_advantages(u.st, u.f64_cur[0].data_ptr(), perm.data_ptr(), n_valid, batch_size, self.num_envs, self.horizon, u.mbn["ddof"],
                                                       adv_table.data_ptr(), u.mb_stats[u.mb_epochs].data_ptr())
                    u.mb_epochs += 1
            if u.demo is not None:                                                   # this epoch's demonstration rows, from the setting's own stream: one upload
                drawn = self.demonstration_rows_drawn(u.demo, db.size, steps_per_epoch)
                u.demo_rows.extend(drawn)
                drawn_dev = torch.from_numpy(drawn).to(device)
            for i in range(0, n_valid, batch_size):
                mb = perm[i:i + batch_size]                                          # the last one may be partial (train.py:199-201)
                m = int(mb.numel())
                if u.demo is not None:                                               # one step on the PPO minibatch and the demonstration rows together
                    ppo._demo_rows(self.states, self.actions, self.returns, adv_table, logp_old, self.mean_old if u.klp is not None else None, mb, m, m,
                                   db.states, db.expert_actions, drawn_dev[i // batch_size], md, md, old_values_all=step_kw.get("old_values_all"), coef=u.demo_coef, loss=u.demo["loss"])
                    u.demo_records.append(pdev.demo_losses.clone())
                elif u.klp is not None:                                                # (the penalised step reads the old policy's means next to its log-probabilities)
                    ppo._kl_step(self.states, self.actions, self.returns, adv_table, logp_old, self.mean_old, mb, m, m, old_values=step_kw.get("old_values_all"))
                else:
                    ppo._step_rows(self.states, self.actions, self.returns, adv_table, logp_old, mb, m, m, **step_kw)
                ppo.train_step_counter += 1
                records.append(pdev.losses.clone())
                if u.klp is not None:
                    u.kl_records.append(pdev.kl_losses.clone())
                if clip:
                    clips.append(pdev.grad_clip.clone())
            if observe is not None:                                                  # observe the epoch: all valid rows under the parameters it ended with
                u.clock.lap("sgd")
                u.epochs.append(observe())
                u.epoch_first.append(len(clips))                                     # (the epoch's norms are read back with all the others, behind the last epoch)
                u.clock.lap("stats")
                if u.diag["target_kl"] is not None and u.epochs[-1]["approx_kl"] > u.diag["target_kl"]:
                    u.stopped = True
                    break

    def _kl_penalty_result(self, u, out):
        """Behind the last epoch: the exact KL(pi_old || pi_theta) over all valid rows under the parameters the update ended with (mi_ppo_kl_stats_idx in the 4096-row
        chunks of the diagnostics pass, one readback), then the coefficient's adaptation on the host (PPO.adapt_kl_penalty)."""
        import torch
        from mi355.ppo_device import N_KL_STATS, kl_stats_summary
        pdev, device, chunk = self.ppo._need_dev(), self.device, 4096
        with u.clock.stage("kl_stats"):
            valid_dev = torch.from_numpy(u.valid).to(device)
            sums = torch.zeros(N_KL_STATS, dtype=torch.float64, device=device)
            scratch = torch.empty(pdev.kl_stats_scratch_doubles(min(u.n_valid, chunk)), dtype=torch.float64, device=device)
            for lo in range(0, u.n_valid, chunk):
                rows = valid_dev[lo:lo + chunk]
                pdev.kl_stats(self.states, self.mean_old, rows, int(rows.numel()), sums, scratch, accumulate=lo > 0)
            kl = kl_stats_summary(sums.cpu().numpy())                                # the one readback
            kls = torch.stack(u.kl_records).cpu().numpy() if u.kl_records else np.zeros((0, 2), np.float32)
        for rec, row in zip(out["losses"], kls):
            rec["kl"], rec["kl_penalty"] = float(row[0]), float(row[1])
        out["kl"], out["kl_coef"] = kl, float(u.kl_coef)
        adapt = self.ppo.kl_target is not None and bool(np.isfinite(kl["kl"])) and kl["kl"] >= 0
        out["kl_coef_next"] = float(self.ppo.adapt_kl_penalty(kl["kl"])) if adapt else float(self.ppo.kl_penalty)
        out["kl_adapted"] = bool(adapt)

    def _demonstration_result(self, u, out):
        """Behind the last epoch: every step's demonstration scalars and rows (one readback), then the coefficient's decay."""
        import torch
        dl = torch.stack(u.demo_records).cpu().numpy() if u.demo_records else np.zeros((0, 3), np.float32)
        out["demo_losses"] = [{"demo_loss": float(r[0]), "mean_sq_error": float(r[2])} for r in dl]
        out["demo_rows"] = [np.array(r, np.int32) for r in u.demo_rows]
        out["demo_coef"] = float(u.demo_coef)
        u.demo["coef"] = float(u.demo_coef * u.demo["decay"])
        out["demo_coef_next"] = u.demo["coef"]

    def _minibatch_norm_result(self, u, out):
        E, T = self.num_envs, self.horizon                                           # one readback behind the last epoch; only the epochs that ran
        out["minibatch_adv_stats"] = u.mb_stats[:u.mb_epochs].reshape(-1, 3).cpu().numpy()
        table = self._minibatch_advantages.view(E, T + 1)[:, :T].cpu().numpy()
        out["minibatch_advantages"] = np.where(u.recorded & (u.mb_epochs > 0), table, np.float32(np.nan)).astype(np.float32)

    def _stats_pass(self, u):
        """The statistics pass of update_with_diagnostics -> observe(): the pass over all valid rows in chunks of 4096 and the epoch's one readback -> the epoch's dict.
        With value clipping on the pass also writes V per table row (_values_new), mi_ppo_value_clip_stats runs over the same chunks, and its sums sit behind the others.
        With dual clip on (PPO.set_dual_clip) it also writes log pi_theta per table row (_logp_new), mi_ppo_dual_clip_stats runs over the same chunks on that table, the
        cache of log pi_old and the advantage table the epoch's steps gathered from (the minibatch table with per-minibatch normalisation), and its sums come last."""
        import torch
        from mi355.ppo_device import N_DUAL_CLIP_STATS, N_STATS, N_VCLIP_STATS, dual_clip_summary, update_stats_summary, value_clip_summary
        pdev, device, vclip, chunk = self.ppo._need_dev(), self.device, u.vclip, 4096
        dual = getattr(self.ppo, "dual_clip", None)
        valid_dev = torch.from_numpy(u.valid).to(device)
        n_v = 0 if vclip is None else N_VCLIP_STATS
        sums = torch.zeros(N_STATS + n_v + (0 if dual is None else N_DUAL_CLIP_STATS), dtype=torch.float64, device=device)
        stats, vstats, dstats, value_out = sums[:N_STATS], sums[N_STATS:N_STATS + n_v], sums[N_STATS + n_v:], None
        stats_kw = {}
        if dual is not None:
            dscratch = torch.empty(pdev.dual_clip_scratch_doubles(min(u.n_valid, chunk)), dtype=torch.float64, device=device)
            if getattr(self, "_logp_new", None) is None:
                self._logp_new = torch.zeros(self.n_table_rows, device=device)
            stats_kw["logp_new_out"] = self._logp_new
        if vclip is not None:
            vscratch = torch.empty(pdev.value_clip_scratch_doubles(min(u.n_valid, chunk)), dtype=torch.float64, device=device)
            if getattr(self, "_values_new", None) is None:
                self._values_new = torch.zeros(self.n_table_rows, device=device)
            value_out = self._values_new
        stats_scratch = torch.empty(pdev.stats_scratch_doubles(min(u.n_valid, chunk)), dtype=torch.float64, device=device)

        def observe():
            for lo in range(0, u.n_valid, chunk):
                rows = valid_dev[lo:lo + chunk]
                pdev.update_stats(self.states, self.actions, self.returns, self.logp_old, rows, int(rows.numel()), stats, stats_scratch, accumulate=lo > 0,
                                  value_out=value_out, **stats_kw)
                if vclip is not None:
                    pdev.value_clip_stats(value_out, self.values, self.returns, rows, int(rows.numel()), vclip, vstats, vscratch, accumulate=lo > 0)
                if dual is not None:
                    pdev.dual_clip_stats(self._logp_new, self.logp_old, u.adv_table, rows, int(rows.numel()), self.ppo.epsilon, dual, dstats, dscratch, accumulate=lo > 0)
            both = sums.cpu().numpy()                                                # the epoch's one readback
            epoch = update_stats_summary(both[:N_STATS])
            if vclip is not None:
                epoch.update(value_clip_summary(both[N_STATS:N_STATS + n_v]))
            if dual is not None:
                epoch.update(dual_clip_summary(both[N_STATS + n_v:]))
            return epoch
        return observe

    def _result(self, u):
        """The keys of every update -- the loss records, the finish call's outputs as [num_envs, T] arrays, NaN beyond a row's length -- and what the SGD loop recorded
        with gradient clipping or diagnostics on."""
        import torch
        E, T, lengths = self.num_envs, self.horizon, u.lengths
        losses = torch.stack(u.records).cpu().numpy() if u.records else np.zeros((0, 5), np.float32)
        u.clock.lap("sgd")
        keys = ("policy_loss", "value_loss", "entropy_loss", "loss", "prob_ratio")
        f64 = u.f64.cpu().numpy()
        v_all = self.values.view(E, T + 1).cpu().numpy()
        values = np.where(u.recorded, v_all[:, :T], np.float32(np.nan)).astype(np.float32)
        out = {"losses": [dict(zip(keys, (float(x) for x in row))) for row in losses], "lengths": lengths, "raw_advantages": f64[0], "returns": f64[1],
               "advantages": f64[2], "values": values, "bootstrap_values": np.where(lengths > 0, v_all[np.arange(E), lengths], np.float32(np.nan)).astype(np.float32),
               "samples": u.n_valid}
        if self.ppo.max_grad_norm is not None:
            gc = torch.stack(u.clips).cpu().numpy() if u.clips else np.zeros((0, 4), np.float32)
            out["grad_norms"], out["clip_scales"] = gc[:, 0].astype(np.float32).copy(), gc[:, 1].astype(np.float32).copy()
            for e, lo, hi in zip(u.epochs, u.epoch_first[:-1], u.epoch_first[1:]):   # (diagnostics)  NaN norms count as the maximum (np.max propagates them)
                e["grad_norm_max"] = float(gc[lo:hi, 0].max()) if hi > lo else float("nan")
                e["clipped_steps"] = int((gc[lo:hi, 1] < 1.0).sum())
        if u.diag is not None:
            out["epochs"], out["epochs_run"], out["stopped_early"] = u.epochs, len(u.epochs), u.stopped
        return out

    def _observation_stats(self, u, on, out):
        with u.clock.stage("observation_stats"):
            batch = self._obs_norm_stats(u.valid, 0 if on["frozen"] else 1, "update")
        out["observation_rms"] = _obs_norm_rms(on)
        out["observation_clip_fraction"] = batch[2] / u.n_valid


class ContinuousRolloutBuffer(RolloutBuffer):
    """RolloutBuffer whose lanes go on after a done (see the module docstring): every environment steps `horizon` times per update, a simulator that reports done is
    stepped again with its reset observation, and update() finishes the lanes segment by segment (mi_rollout_finish_segments).  Same tables and recording step, and
    `final_values` (fp32, num_envs (horizon + 1) entries like the other tables): entry r holds the value of the final observation of the episode that truncate() ended
    at table row r."""

    _rows_class = SegmentedRows

    def __init__(self, vae, ppo, num_envs, horizon, seed=None, io=None):
        self._init(vae, ppo, num_envs, horizon, seed, io, 1)

    def _init(self, vae, ppo, num_envs, horizon, seed, io, latent_stack):
        import torch
        super()._init(vae, ppo, num_envs, horizon, seed, io, latent_stack)
        self.final_values = torch.zeros(self.n_table_rows, device=self.device)
        # advantage recomputation (set_advantage_recomputation): the state rows of the final observations, the scratch tables the recording call fills beside them, and
        # the refreshed final values -- allocated when the setting is turned on / by the first update that needs it
        self.final_states = self._final_actions = self._final_raw_states = self.final_values_now = None

    def set_advantage_recomputation(self, on=True):
        """RolloutBuffer.set_advantage_recomputation.  With the setting on truncate() is a greedy recording call that keeps the final observation's state row in
        `final_states` (at the truncated step's row, like `final_values`), and every refresh also values those rows into `final_values_now`, which its finish call
        bootstraps the truncated segments from.  `final_values` stays the recorded table."""
        import torch
        super().set_advantage_recomputation(on)
        if not self._adv_recompute:
            self.final_states = self._final_actions = self._final_raw_states = self.final_values_now = None
            return
        if self.final_states is None:
            n = self.n_table_rows
            self.final_states = torch.zeros(n, int(self.ppo.input_dim), device=self.device)
            self._final_actions = torch.zeros(n, int(self.ppo.num_actions), device=self.device)
            self.final_values_now = torch.zeros(n, device=self.device)

    def bootstrap(self, frames_u8, measurements, env_ids=None):
        """RolloutBuffer.bootstrap; env_ids None: rows.needs_bootstrap() -- a lane whose last step reported done or was truncated needs none (given one, it is recorded and
        never read).  With no such lane and no frames the call does nothing."""
        if env_ids is None:
            env_ids = self.rows.needs_bootstrap()
        if len(env_ids) == 0 and (frames_u8 is None or len(frames_u8) == 0):         # (the loop's frames[need] with every lane ending in a done)
            return None
        return super().bootstrap(frames_u8, measurements, env_ids)

    def truncate(self, final_frames_u8, final_measurements, env_ids=None):
        """The episodes of these environments (None: 0 .. n-1) stopped at their last counted step WITHOUT being terminal, and their lanes go on with a reset observation:
        call it after outcome() (done False) and before these lanes' next step, with the final observation of the stopped episodes.  One value-only device call
        (mi_rollout_value_batch_rec; with observation normalisation on, mi_rollout_value_batch_norm) leaves V(final observation) in final_values at the row of that step; update() bootstraps the segment from it.  -> float32 [n].
        With advantage recomputation on (set_advantage_recomputation) it is a greedy recording call instead (mi_rollout_step_batch_rec and its forms, as bootstrap():
        the history is read and not advanced) that also keeps the state row, in `final_states` at the same row; the value it returns is the same quantity."""
        f, n, meas, _ = self._step.check(final_frames_u8, final_measurements, True, None)
        rows = self.rows.truncate_rows(env_ids, n)
        if getattr(self, "_adv_recompute", False):
            # advantage recomputation: a greedy recording call, as bootstrap() is -- the state row stays on the device (final_states) for the refreshes to value; the
            # action it writes is never read, the history is read and not advanced
            if self._obs_norm is not None and self._final_raw_states is None:
                import torch
                self._final_raw_states = torch.zeros(self.n_table_rows, int(self.ppo.input_dim), device=self.device)
            values = self._step.record(f, n, meas, None, True, rows, self.final_states, self._final_actions, self.final_values, self._final_raw_states,
                                       lanes=self._lanes(env_ids, n), advance=False)[1].astype(np.float32)
            if self._stacked():
                self._step.fresh[self.rows.env_ids(env_ids, n)] = True
            return values
        if not self._stacked():
            return self._step.record_value(f, n, meas, rows, self.final_values)
        lanes = self.rows.env_ids(env_ids, n)                                        # latent stacking: the final observation is valued on the episode's history, the lane's next step starts afresh
        values = self._step.record_value_lanes(f, n, meas, rows, self.final_values, lanes)
        self._step.fresh[lanes] = True
        return values

    def update(self, gamma=0.99, lam=0.95, num_epochs=3, batch_size=32, normalize="segment", stage_times=None):
        """RolloutBuffer.update with one mi_rollout_finish_segments call for the finish (mi_rollout_finish_segments_boot, which also takes the per-segment bootstrap
        source, if and only if a step of this collection was truncated).  normalize: "segment" (train.py:176-177 on every segment alone, the reference's semantics) or
        "batch" (mean and population std over all samples of the update: a 1-step tail segment's advantage is not forced to 0).  Returns RolloutBuffer.update's keys,
        `segments` (SegmentedRows.segments()), `segment_truncated` (SegmentedRows.segment_truncated()) and `final_values`, float32 [num_envs, T]: the value a truncated
        step's segment bootstrapped from, NaN where no truncation was recorded; `bootstrap_values` is NaN for lanes whose last step reported done or was truncated."""
        return self._run_update(gamma, lam, num_epochs, batch_size, stage_times, None, normalize)

    def update_with_diagnostics(self, gamma=0.99, lam=0.95, num_epochs=3, batch_size=32, normalize="segment", stage_times=None, target_kl=None):
        """This class's update() with RolloutBuffer.update_with_diagnostics' per-epoch statistics pass, `epochs` / `epochs_run` / `stopped_early` and target_kl."""
        return self._run_update(gamma, lam, num_epochs, batch_size, stage_times, _diagnostics(type(self).__name__, target_kl), normalize)

    def _run_update(self, gamma, lam, num_epochs, batch_size, stage_times, diag, normalize="segment"):
        if normalize not in ("segment", "batch"):
            raise ValueError("ContinuousRolloutBuffer.update: normalize is 'segment' or 'batch'")
        segs = self.rows.segments()
        truncs = self.rows.truncs.copy()
        seg_trunc = self.rows._truncated(segs)                                      # = segment_truncated(), from the one segments() walk

        def finish(st, r, d, lengths, f64, now=False, vt=None):
            import torch
            n_seg, T = int(segs.shape[0]), self.horizon
            desc = [segs[:, 0] * (T + 1) + segs[:, 1], segs[:, 2]]                   # table row of the first slot | length
            if truncs.any():
                desc.append(seg_trunc)                                               # | bootstraps from final_values
            desc = torch.from_numpy(np.stack(desc).astype(np.int32)).to(self.device)
            batch = normalize == "batch"
            scratch = torch.empty(int(self.L.mi_rollout_finish_segments_scratch_doubles(n_seg)), dtype=torch.float64, device=self.device) if batch else None
            args = (st, (self.values_now if now else self.values).data_ptr(), r.data_ptr(), d.data_ptr(), desc[0].data_ptr(), desc[1].data_ptr(), n_seg, self.num_envs, T, float(gamma), float(lam),
                    1 if batch else 0, milib.ptr(scratch), self.returns.data_ptr(), self.advantages.data_ptr(), f64[0].data_ptr(), f64[1].data_ptr(), f64[2].data_ptr())
            if vt is not None:                                                       # a V-trace refresh: the same segments, the segment kernels' successor rule
                boot = truncs.any()
                self.L.mi_rollout_finish_vtrace(st, self.values_now.data_ptr(), vt["logp_now"].data_ptr(), vt["logp_old"].data_ptr(), *args[2:11], vt["rho_bar"], vt["c_bar"], 0,
                                                *args[11:], vt["weights"].data_ptr(), self.final_values_now.data_ptr() if boot else None, desc[2].data_ptr() if boot else None)
            elif truncs.any():
                self.L.mi_rollout_finish_segments_boot(*args, (self.final_values_now if now else self.final_values).data_ptr(), desc[2].data_ptr())
            else:
                self.L.mi_rollout_finish_segments(*args)
        last_done = self.rows._last_done()
        out = self._update(finish, num_epochs, batch_size, stage_times, diag, gamma, truncs)
        out["segments"], out["segment_truncated"] = segs, seg_trunc
        out["bootstrap_values"] = np.where(last_done, np.float32(np.nan), out["bootstrap_values"]).astype(np.float32)
        final = np.full(truncs.shape, np.nan, np.float32)
        if truncs.any():
            final[truncs] = self.final_values.view(self.num_envs, self.horizon + 1)[:, :self.horizon].cpu().numpy()[truncs]
        out["final_values"] = final
        if out.get("recomputed_epochs"):                                             # advantage recomputation: what the last refresh's truncated segments bootstrapped from
            now = np.full(truncs.shape, np.nan, np.float32)
            if truncs.any():
                now[truncs] = self.final_values_now.view(self.num_envs, self.horizon + 1)[:, :self.horizon].cpu().numpy()[truncs]
            out["refreshed_final_values"] = now
        return out

    def _recompute_rows(self, u):
        """RolloutBuffer._recompute_rows without the bootstrap slot of a lane whose last step reported done or was truncated: nothing behind it is read, and no
        bootstrap() need have recorded a state there."""
        lanes = np.nonzero((u.lengths > 0) & ~self.rows._last_done())[0]
        return np.concatenate([u.valid, (self.rows._base[lanes] + u.lengths[lanes]).astype(np.int32)]).astype(np.int32)

    def _recompute_extra(self, u):
        """The truncated steps' final observations: one more mi_ppo_values_idx call, over `final_states` at the truncated rows into `final_values_now`."""
        import torch
        if getattr(u, "trunc_rows", None) is None:
            e, t = np.nonzero(self.rows.truncs)
            u.trunc_rows = torch.from_numpy((e * (self.horizon + 1) + t).astype(np.int32)).to(self.device)
            self.final_values_now.copy_(self.final_values)
        if int(u.trunc_rows.numel()):
            self.ppo._need_dev().values_idx(self.final_states, u.trunc_rows, int(u.trunc_rows.numel()), self.final_values_now)


class _DemonstrationStep(BatchedRolloutStep):
    """The step of a DemonstrationBuffer: the recording step under the buffer's name."""

    _who = "DemonstrationBuffer"
    _row_ints = 1


def clone_losses_of(records):
    """The loss records of clone steps (the first five floats of the losses buffer each) -> [{clone_loss, value_loss, loss, mean_sq_error}, ...]."""
    return [{"clone_loss": float(r[0]), "value_loss": float(r[1]), "loss": float(r[3]), "mean_sq_error": float(r[4])} for r in records]


class DemonstrationBuffer:
    """Behaviour cloning from demonstrations (CARLA's autopilot, a human driver): up to `capacity` (camera frame, measurements, expert action[, return]) rows.
    add() turns the frames into the policy's state rows on the device -- the batched recording step, greedy, in chunks of at most `chunk` frames -- and keeps them in
    the device table `states` [capacity, input_dim]; the expert's actions and the returns go to the tables `expert_actions` [capacity, A] and `returns` [capacity],
    the policy's own greedy actions and values at recording time to `policy_actions` / `policy_values`.  clone() trains the policy on shuffled minibatches of the
    rows (PPO._clone_rows: mi_ppo_clone_step with the in-kernel gather), and the value net if and only if returns were added; evaluate() scores the current policy
    against the expert in float64.  Afterwards PPO training continues from the warm-started policy through a rollout buffer.  Latent stacking is not supported."""

    def __init__(self, vae, ppo, capacity, chunk=64, seed=None, io=None):
        import torch
        for name, v, hi in (("capacity", capacity, 1 << 24), ("chunk", chunk, MAX_ENVS)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= hi:
                raise ValueError("DemonstrationBuffer: %s is an int in [1, %d], got %r" % (name, hi, v))
        self.capacity, self.chunk = int(capacity), int(chunk)
        self.vae, self.ppo = vae, ppo
        self._step = _DemonstrationStep(vae, ppo, self.chunk, seed=seed, io=io)     # (raises before anything touches a device where the sizes do not fit)
        self.io, self.device, self.L = self._step.io, self._step.device, self._step.L
        self.A = int(ppo.num_actions)
        n = self.capacity
        self.states = torch.zeros(n, int(ppo.input_dim), device=self.device)
        self.policy_actions = torch.zeros(n, self.A, device=self.device)
        self.policy_values = torch.zeros(n, device=self.device)
        self.expert_actions = torch.zeros(n, self.A, device=self.device)
        self.returns = torch.zeros(n, device=self.device)
        self.raw_states = None                                                       # the raw rows beside normalised ones (set_observation_normalization)
        self.reset()

    @classmethod
    def stacked(cls, vae, ppo, capacity, latent_stack, chunk=64, seed=None, io=None):
        """The demonstration buffer has no stacked form: ValueError for anything but latent_stack = 1."""
        if isinstance(latent_stack, (bool, np.bool_)) or not isinstance(latent_stack, (int, np.integer)) or int(latent_stack) != 1:
            raise ValueError("DemonstrationBuffer: latent stacking is not supported (a stacked policy's demonstrations need their episodes' order): latent_stack must be 1")
        return cls(vae, ppo, capacity, chunk=chunk, seed=seed, io=io)

    def reset(self):
        """Empties the buffer; the tables keep their contents and are overwritten by the next rows."""
        self.size = 0
        self.has_returns = None                                                      # None until the first add() decides it

    def set_observation_normalization(self, state_dict):
        """Frozen observation statistics (a rollout buffer's observation_normalization_state(); None: off) are applied at encoding time by every add() from now on:
        `states` then holds the normalised rows, as the buffer that produced the statistics trains on, and `raw_states` the raw ones."""
        import torch
        self._step.set_observation_normalization(state_dict)
        if state_dict is not None and self.raw_states is None:
            self.raw_states = torch.zeros(self.capacity, int(self.ppo.input_dim), device=self.device)

    def check_add(self, frames_u8, measurements, expert_actions, returns):
        """The host-side checks of add() -> (frames, n, measurements, expert actions float32 [n, A], returns float32 [n] or None).  ValueError, before any launch."""
        who = "DemonstrationBuffer.add"
        f = np.asarray(frames_u8)
        fb = self._step.frame_bytes
        if f.dtype != np.uint8 or f.ndim < 1 or f.shape[0] < 1 or f.size != f.shape[0] * fb:
            raise ValueError("%s: expected uint8 frames [n, ...] of %d bytes each, n >= 1" % (who, fb))
        n = int(f.shape[0])
        if self.size + n > self.capacity:
            raise ValueError("%s: %d rows on top of %d exceed the capacity of %d" % (who, n, self.size, self.capacity))
        meas = np.asarray(measurements, np.float64)
        if meas.shape != (n, self._step.n_meas):
            raise ValueError("%s: expected measurements [%d, %d]" % (who, n, self._step.n_meas))
        a = np.asarray(expert_actions)
        if a.dtype.kind not in "fiu" or a.shape != (n, self.A):
            raise ValueError("%s: expected expert_actions [%d, %d]" % (who, n, self.A))
        a = np.ascontiguousarray(a, np.float32)
        if not np.isfinite(a).all():
            raise ValueError("%s: expert_actions holds values that are not finite" % who)
        lo, hi = np.asarray(self.ppo.action_low, np.float32), np.asarray(self.ppo.action_high, np.float32)
        if (a < lo).any() or (a > hi).any():
            raise ValueError("%s: expert_actions outside [action_low, action_high] = [%s, %s]: the expert's units are not the policy's" % (who, lo.tolist(), hi.tolist()))
        if self.has_returns is not None and (returns is not None) != self.has_returns:
            raise ValueError("%s: returns were %s by the earlier add() calls and are %s now: all rows carry returns or none does (reset() starts over)"
                             % (who, "given" if self.has_returns else "not given", "given" if returns is not None else "not given"))
        r = None
        if returns is not None:
            r = np.asarray(returns)
            if r.dtype.kind not in "fiu" or r.reshape(-1).shape != (n,):
                raise ValueError("%s: expected returns [%d]" % (who, n))
            r = np.ascontiguousarray(r.reshape(-1), np.float32)
            if not np.isfinite(r).all():
                raise ValueError("%s: returns holds values that are not finite" % who)
        return f.reshape(n, -1), n, meas, a, r

    def add(self, frames_u8, measurements, expert_actions, returns=None):
        """Appends n demonstration rows: frames_u8 uint8 [n, H, W, 3], measurements [n, k], expert_actions [n, A] inside [action_low, action_high], returns [n] or
        None (for every add() alike).  -> the table rows, int64 [n]."""
        import torch
        f, n, meas, a, r = self.check_add(frames_u8, measurements, expert_actions, returns)
        step, lo = self._step, self.size
        for i in range(0, n, self.chunk):
            c = min(self.chunk, n - i)
            rows = np.arange(lo + i, lo + i + c, dtype=np.int32)
            step.record(f[i:i + c], c, meas[i:i + c], None, True, table_rows=rows, states=self.states, actions=self.policy_actions, values=self.policy_values,
                        raw_states=self.raw_states)
        self.expert_actions[lo:lo + n].copy_(torch.from_numpy(a))
        if r is not None:
            self.returns[lo:lo + n].copy_(torch.from_numpy(r))
        self.has_returns = r is not None
        self.size = lo + n
        return np.arange(lo, lo + n)

    def clone(self, num_epochs=1, batch_size=32, loss="nll"):
        """Epochs of np.random.shuffle'd minibatches over the rows (the legacy numpy RNG, as the rollout buffers; the last minibatch of an epoch may be partial), each
        one PPO._clone_rows call.  The value net is fitted if and only if returns were added.  -> {"losses": [{clone_loss, value_loss, loss, mean_sq_error}, ...],
        "samples"} and, with gradient clipping on, "grad_norms" / "clip_scales"."""
        import torch
        from mi355 import dist as midist
        who = "DemonstrationBuffer"
        if midist.world_size() > 1:
            raise ValueError(who + ".clone: single rank only (ragged rows give ranks different numbers of gradient all-reduces)")
        if isinstance(batch_size, (bool, np.bool_)) or isinstance(num_epochs, (bool, np.bool_)) or int(batch_size) < 1 or int(num_epochs) < 0:
            raise ValueError(who + ".clone: batch_size >= 1 and num_epochs >= 0")
        milib.clone_kind(loss, who + ".clone")
        if self.size < 1:
            raise ValueError(who + ".clone: the buffer is empty")
        ppo, pdev, n, batch_size = self.ppo, self.ppo._need_dev(), self.size, int(batch_size)
        returns = self.returns if self.has_returns else None
        clip = ppo.max_grad_norm is not None
        records, clips = [], []
        for _ in range(int(num_epochs)):
            indices = np.arange(n)
            np.random.shuffle(indices)
            perm = torch.from_numpy(indices.astype(np.int32)).to(self.device)
            for i in range(0, n, batch_size):
                mb = perm[i:i + batch_size]
                m = int(mb.numel())
                ppo._clone_rows(self.states, self.expert_actions, returns, mb, m, m, loss=loss)
                ppo.train_step_counter += 1
                records.append(pdev.losses[:5].clone())
                if clip:
                    clips.append(pdev.grad_clip.clone())
        losses = torch.stack(records).cpu().numpy() if records else np.zeros((0, 5), np.float32)
        out = {"losses": clone_losses_of(losses), "samples": n}
        if clip:
            gc = torch.stack(clips).cpu().numpy() if clips else np.zeros((0, 4), np.float32)
            out["grad_norms"], out["clip_scales"] = gc[:, 0].astype(np.float32).copy(), gc[:, 1].astype(np.float32).copy()
        return out

    def evaluate(self):
        """The current policy against the expert over all rows: PpoDevice.predict (greedy) in chunks -- theta_old and the training state are not touched --, then in
        float64 on the host: {"samples", "nll": mean_m sum_a (z^2 / 2 + logstd + log(2 pi) / 2), "mean_sq_error": mean_m sum_a (mean - a_E)^2,
        "max_abs_error": float64 [A], "means": float32 [n, A]}."""
        import torch
        if self.size < 1:
            raise ValueError("DemonstrationBuffer.evaluate: the buffer is empty")
        pdev, n = self.ppo._need_dev(), self.size
        mean = torch.empty(n, self.A, device=self.device)
        value = torch.empty(n, device=self.device)
        chunk = max(self.chunk, 256)
        for lo in range(0, n, chunk):
            hi = min(lo + chunk, n)
            pdev.predict(self.states[lo:hi], hi - lo, None, True, mean[lo:hi], value[lo:hi])
        o, cnt = pdev.layout["policy/action_logstd"]
        logstd = pdev.params[o:o + cnt].cpu().numpy().astype(np.float64)
        mu, a_e = mean.cpu().numpy(), self.expert_actions[:n].cpu().numpy().astype(np.float64)
        d = mu.astype(np.float64) - a_e
        z = d / np.exp(logstd)
        return {"samples": n, "nll": float((0.5 * z * z + logstd + 0.5 * np.log(2.0 * np.pi)).sum(axis=1).mean()), "mean_sq_error": float((d * d).sum(axis=1).mean()),
                "max_abs_error": np.abs(d).max(axis=0), "means": mu}
