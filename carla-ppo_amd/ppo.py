"""ppo — drop-in for the reference's ppo.py (PPO class surface) on MI355X through libmi355_carla.so.

Reference symbols mirrored (file:line in the reference checkout):
    PolicyGraph            ppo.py:11-66     (fused into the native engine: two 67-500-300 MLPs, Gaussian head)
    PPO.__init__           ppo.py:73-190    init_session :192-200   save :202-205   load_latest_checkpoint :207-216
    train                  ppo.py:218-229   (alias: learn; explicit single step: train_step)
    predict                ppo.py:231-251   get_*_idx :253-260      write_*_summary :262-273   update_old_policy :275-276

Host code is plumbing (numpy in / numpy out, torch tensors as HBM handles).  All arithmetic runs in HIP kernels;
there is no CPU fallback — init_session() raises without a GPU or without the built library.
"""
import os

import numpy as np

from mi355 import checkpoint as ckpt
from mi355 import dist as midist
from mi355 import lib as milib
from mi355.init import init_ppo, ppo_variables

ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON = 0.9, 0.999, 1e-8


def _max_grad_norm_from_env():
    """MI355_PPO_MAX_GRAD_NORM (unset or empty: off) -> None or a positive float; anything else raises ValueError."""
    text = os.environ.get("MI355_PPO_MAX_GRAD_NORM", "").strip()
    if not text:
        return None
    try:
        return milib.max_grad_norm_value(float(text), "MI355_PPO_MAX_GRAD_NORM=%r" % text)
    except ValueError:
        raise ValueError("MI355_PPO_MAX_GRAD_NORM=%r: expected a positive float or inf" % text) from None


def _dual_clip_from_env():
    """MI355_PPO_DUAL_CLIP (unset or empty: off) -> None or a float > 1 (inf included); anything else raises ValueError."""
    text = os.environ.get("MI355_PPO_DUAL_CLIP", "").strip()
    if not text:
        return None
    try:
        return milib.dual_clip_value(float(text), "MI355_PPO_DUAL_CLIP=%r" % text)
    except ValueError:
        raise ValueError("MI355_PPO_DUAL_CLIP=%r: expected a float > 1 or inf" % text) from None


def _wide_inputs_from_env():
    """MI355_PPO_WIDE_INPUTS (unset or empty: off) -> False for "0", True for "1"; anything else raises ValueError."""
    text = os.environ.get("MI355_PPO_WIDE_INPUTS", "").strip()
    if text in ("", "0"):
        return False
    if text == "1":
        return True
    raise ValueError("MI355_PPO_WIDE_INPUTS=%r: expected 0 or 1" % text)


def _kl_coef_from_env():
    """MI355_PPO_KL_COEF (unset or empty: off) -> None or a finite float >= 0 (a fixed coefficient, no target); anything else raises ValueError."""
    text = os.environ.get("MI355_PPO_KL_COEF", "").strip()
    if not text:
        return None
    try:
        return milib.kl_penalty_value(float(text), "MI355_PPO_KL_COEF=%r" % text)
    except ValueError:
        raise ValueError("MI355_PPO_KL_COEF=%r: expected a finite float >= 0" % text) from None


def adapted_kl_coef(coef, target, kl):
    """The PPO paper's rule (Schulman et al. 2017, section 4): kl < target / 1.5 halves the coefficient, kl > 1.5 target doubles it, both comparisons strict;
    target None leaves it.  kl: the mean KL(pi_old || pi_theta) behind the update's last epoch, finite and >= 0 (else ValueError)."""
    if isinstance(kl, bool) or not isinstance(kl, (int, float, np.floating, np.integer)) or not (kl >= 0 and kl < float("inf")):
        raise ValueError("adapt_kl_penalty: kl is a finite float >= 0, got %r" % (kl,))
    if target is None:
        return float(coef)
    if kl < target / 1.5:
        return float(coef) / 2.0
    if kl > 1.5 * target:
        return float(coef) * 2.0
    return float(coef)


def _adam_alpha(lr, b1p, b2p):
    one = np.float32(1.0)
    return np.float32(np.float32(lr) * np.sqrt(one - np.float32(b2p), dtype=np.float32) / (one - np.float32(b1p)))


class PPO():
    """Proximal policy optimisation model (reference ppo.py:68-276)."""

    def __init__(self, input_shape, action_space,
                 learning_rate=3e-4, lr_decay=0.998, epsilon=0.2,
                 value_scale=0.5, entropy_scale=0.01, initial_std=0.4,
                 model_dir="./", seed=None, precision=None):
        # precision of the training step: "fp32" (exact, the default) or "bf16x3" (the GEMM stages on the bf16 matrix pipe as split hi + lo operands,
        # include/mi355_carla.h mi_ppo_set_precision).  MI355_PPO_PRECISION supplies it when the argument is not given; MI355_PRECISION is the VAE's knob
        # and does not apply here.  Not part of a checkpoint: weights and optimiser state are fp32 in both modes.
        self.precision = milib.ppo_precision_name(precision or os.environ.get("MI355_PPO_PRECISION", "fp32"))
        # global-norm gradient clipping in front of Adam (set_max_grad_norm): None = off.  MI355_PPO_MAX_GRAD_NORM supplies it when set_max_grad_norm is not called
        # (the reference's train.py builds this object itself).  Not part of a checkpoint.
        self.max_grad_norm = _max_grad_norm_from_env()
        # dual-clip PPO (set_dual_clip): the constant c > 1 that bounds the surrogate of a sample with a negative advantage and a large ratio; None = off.
        # MI355_PPO_DUAL_CLIP supplies it when set_dual_clip is not called.  Not part of a checkpoint.
        self.dual_clip = _dual_clip_from_env()
        # PPO2-style value-function clipping (set_value_clip): None = off.  No environment knob: only the rollout buffers record the old values a clipped step needs.
        # Not part of a checkpoint.
        self.value_clip = None
        # adaptive KL penalty (set_kl_penalty): beta x mean KL(pi_old || pi_theta) added to the clipped surrogate; None = off.  MI355_PPO_KL_COEF supplies a fixed beta
        # when set_kl_penalty is not called.  kl_target: None (beta fixed) or the KL the rollout buffers steer beta towards.  Not part of a checkpoint's state_dict():
        # kl_penalty_state() / load_kl_penalty_state() carry it.
        self.kl_penalty = _kl_coef_from_env()
        self.kl_target = None
        # demonstration term (set_demonstration_loss): c_d x clone_loss of a minibatch of demonstration rows added to the PPO objective inside the same step
        # (_demo_rows); None = off.  demo_kind: "nll" / "mse".  Not part of a checkpoint.
        self.demo_coef, self.demo_kind = None, "nll"
        # wide inputs (set_wide_inputs): the fused kernels for a policy of more than 96 inputs (a VAE of more than 93 latents).  MI355_PPO_WIDE_INPUTS=1 supplies it
        # when set_wide_inputs is not called (the reference's train.py builds this object itself).  Routing only; not part of a checkpoint.
        self.wide_inputs = _wide_inputs_from_env()
        self.input_dim = int(np.asarray(input_shape).reshape(-1)[0])
        self.num_actions = int(action_space.shape[0])
        self.action_low = np.asarray(action_space.low, np.float32).reshape(-1)
        self.action_high = np.asarray(action_space.high, np.float32).reshape(-1)
        self.learning_rate_value, self.lr_decay = learning_rate, lr_decay
        self.epsilon, self.value_scale, self.entropy_scale = epsilon, value_scale, entropy_scale
        self.initial_std, self.seed = initial_std, seed
        self._variables = ppo_variables(self.input_dim, self.num_actions)
        self._init_values = None

        # counters (ppo.py:95-98)
        self.train_step_counter = 0
        self.predict_step_counter = 0
        self.episode_counter = 0
        self.beta1_power, self.beta2_power = np.float32(ADAM_BETA1), np.float32(ADAM_BETA2)
        self._metric_sums, self._metric_n = {}, 0
        self.dev = None
        self.sess = None
        self.train_writer = None
        self._noise_offset = 0                                 # N(0,1) values drawn so far from this agent's Philox stream (predict)

        # Setup model saver and dirs (ppo.py:183-190)
        self.model_dir = model_dir
        self.checkpoint_dir = "{}/checkpoints/".format(self.model_dir)
        self.log_dir = "{}/logs/".format(self.model_dir)
        self.video_dir = "{}/videos/".format(self.model_dir)
        self.dirs = [self.checkpoint_dir, self.log_dir, self.video_dir]
        for d in self.dirs:
            os.makedirs(d, exist_ok=True)

    # ------------------------------------------------------------------ session / engine
    def init_session(self, sess=None, init_logging=True):
        from mi355.ppo_device import PpoDevice
        self.sess = sess if sess is not None else self
        if self.seed is None:                                  # train.py's np.random.seed(--seed) drives initialisation and sampling (mi355.init.seed_from_numpy_state)
            from mi355.init import seed_from_numpy_state
            self.seed = seed_from_numpy_state()
        self.dev = PpoDevice(self.input_dim, self.num_actions, self.action_low, self.action_high,
                             self.epsilon, self.value_scale, self.entropy_scale, precision=self.precision, wide_inputs=int(self.wide_inputs))
        self.dev.set_max_grad_norm(self.max_grad_norm)
        self.dev.set_dual_clip(self.dual_clip)
        values = self._init_values or init_ppo(self.seed, self.input_dim, self.num_actions, self.initial_std)
        # policy_old is a separately initialised copy in the reference; the trainer overwrites it with
        # update_old_policy() before the first train() (train.py:192), so it starts as a copy of policy.
        self.dev.load_params(values, {k.replace("policy/", "policy_old/", 1): v for k, v in values.items()})
        if midist.world_size() > 1:
            midist.broadcast(self.dev.params, 0)
            midist.broadcast(self.dev.params_old, 0)
        if init_logging:
            from mi355.summary import SummaryWriter
            self.train_writer = SummaryWriter(self.log_dir)

    def _need_dev(self):
        if self.dev is None:
            raise RuntimeError("call init_session() first")
        return self.dev

    def set_max_grad_norm(self, value):
        """Clip every SGD step's gradient by its global L2 norm over the 13 policy/ variables before Adam (tf.clip_by_global_norm; other libraries' max_grad_norm):
        None switches it off (the default), a positive float switches it on, inf measures the norm and never clips.  Usable before or after init_session(); bool,
        str, 0, a negative value or NaN raise ValueError before anything touches a device.  With it on, every step forms the whole gradient first (the fused chain,
        a sum-of-squares launch, Adam) instead of applying Adam inside the gradient kernels, and last_grad_norm() / the rollout buffers' update() report the norms."""
        self.max_grad_norm = milib.max_grad_norm_value(value, "PPO.set_max_grad_norm")
        if self.dev is not None:
            self.dev.set_max_grad_norm(self.max_grad_norm)

    def set_dual_clip(self, c):
        """Dual-clip PPO (Ye et al. 2020, eq. 5; include/mi355_carla.h, mi_ppo_set_dual_clip): with a constant c > 1 the surrogate of a sample with A < 0 is
        max(min(r A, clip(r) A), c A) -- once the ratio of such a sample has grown past c its term is the constant c A and gives the policy no gradient, where the
        clipped surrogate alone grows with r without bound.  None switches it off (the default), a float > 1 switches it on, inf runs the setting and never
        dual-clips a sample.  Usable before or after init_session(); bool, str, NaN or a value <= 1 raise ValueError before anything touches a device.  train(),
        train_step() and the rollout buffers' update() honour it without further inputs: the setting lives on the engine.  Fused kernels only: a step that would
        take the per-layer path refuses while it is on.  Not part of a checkpoint."""
        self.dual_clip = milib.dual_clip_value(c, "PPO.set_dual_clip")
        if self.dev is not None:
            self.dev.set_dual_clip(self.dual_clip)

    def set_loss_coefficients(self, epsilon=None, value_scale=None, entropy_scale=None):
        """Change the clip range, the value-loss scale and the entropy coefficient of a live model (mi_ppo_set_loss_coefs): a clip-range or entropy schedule that
        keeps parameters, Adam state and tables.  None keeps a value; epsilon is a finite float > 0, value_scale and entropy_scale finite floats >= 0 -- bool, str,
        NaN, inf or a value outside its range raise ValueError before anything changes or touches a device.  Updates the attributes epsilon, value_scale and
        entropy_scale, and the device if there is one; every later step and statistics pass reads the new values."""
        ce, vs, es = milib.loss_coef_values(self.epsilon if epsilon is None else epsilon, self.value_scale if value_scale is None else value_scale,
                                            self.entropy_scale if entropy_scale is None else entropy_scale, "PPO.set_loss_coefficients")
        if self.dev is not None:
            self.dev.set_loss_coefs(ce, vs, es)
        self.epsilon, self.value_scale, self.entropy_scale = ce, vs, es

    def set_wide_inputs(self, on=True):
        """Let the fused kernels take a policy of up to 1024 (padded) inputs instead of 96 -- a VAE of more than 93 latents: train_vae.py --z_dim 128, ConvVAE's own
        default of 512 (include/mi355_carla.h, mi_ppo_set_wide_inputs mode 1).  Off (the default), such a policy trains on the per-layer path, where the in-kernel
        minibatch gather, the cached log pi_old, value clipping, the KL penalty, the update diagnostics and the bf16x3 precision do not exist.  A policy of at most 96
        inputs runs the same launches either way.  Usable before or after init_session(); anything but a bool raises ValueError.  Routing only: it may change between
        two updates and is no part of a checkpoint."""
        if not isinstance(on, bool):
            raise ValueError("PPO.set_wide_inputs: on is True or False, got %r" % (on,))
        self.wide_inputs = on
        if self.dev is not None:
            self.dev.set_wide_inputs(int(on))

    def set_value_clip(self, value):
        """Clip the value loss as the original PPO2 code does (baselines ppo2; clip_vloss / clip_range_vf elsewhere): with eps_v = value the value term of a sample is
        max((V - R)^2, (V_c - R)^2), V_c = V clamped into [V_old - eps_v, V_old + eps_v], V_old the value recorded when the data was collected -- the value net gets no
        gradient from a sample whose value has moved further than eps_v from V_old in the direction of its return.  None switches it off (the default), a positive
        float switches it on, inf runs the clipped step and never clips.  Usable before or after init_session(); bool, str, 0, a negative value or NaN raise
        ValueError before anything touches a device.  The rollout buffers' update() passes the recorded values; train() / train_step() take no old values and refuse
        to run while it is set."""
        self.value_clip = milib.value_clip_value(value, "PPO.set_value_clip")

    def set_kl_penalty(self, coef, target=None):
        """Add the KL penalty of the PPO paper (section 4) to the clipped surrogate: loss += coef x mean_m KL(pi_old || pi_theta)[m], the closed form for this
        diagonal Gaussian policy (include/mi355_carla.h, mi_ppo_train_step_kl); the clip stays as configured.  coef None switches it off (the default), a finite float
        >= 0 switches it on (0: the penalised step that only measures the KL).  target None keeps coef fixed; a finite float > 0 lets the rollout buffers' update()
        adapt it after every update (adapt_kl_penalty).  Usable before or after init_session(); bool, str, NaN, inf or a negative value raise ValueError before
        anything touches a device."""
        coef = milib.kl_penalty_value(coef, "PPO.set_kl_penalty")
        target = milib.kl_target_value(target, "PPO.set_kl_penalty: target")
        if coef is None and target is not None:
            raise ValueError("PPO.set_kl_penalty: a target without a coefficient")
        self.kl_penalty, self.kl_target = coef, target

    def adapt_kl_penalty(self, kl):
        """The paper's rule on the mean KL behind an update's last epoch: kl < target / 1.5 halves beta, kl > 1.5 target doubles it (both strict), else -- or with no
        target -- beta stays.  -> the new beta.  A kl that is not finite or is negative raises ValueError and leaves beta unchanged."""
        if self.kl_penalty is None:
            raise ValueError("PPO.adapt_kl_penalty: the KL penalty is off (set_kl_penalty)")
        self.kl_penalty = adapted_kl_coef(self.kl_penalty, self.kl_target, kl)
        return self.kl_penalty

    def kl_penalty_state(self):
        """{"kl_coef", "kl_target"}: what load_kl_penalty_state restores (beta moves with every adapted update; it is not part of state_dict())."""
        return {"kl_coef": self.kl_penalty, "kl_target": self.kl_target}

    def load_kl_penalty_state(self, d):
        if set(d) != {"kl_coef", "kl_target"}:
            raise ValueError("PPO.load_kl_penalty_state: expected the keys kl_coef and kl_target, got %s" % sorted(d))
        self.set_kl_penalty(d["kl_coef"], d["kl_target"])

    def _kl_step(self, s, a, r, adv, logp_old, mean_old, rows, m_local, m_global, old_values=None):
        """One SGD step through mi_ppo_train_step_kl (the penalty is on): contiguous tensors (rows None) or table rows `rows` (int32 device tensor) of the
        horizon-batch tables; mean_old: the old policy's means, indexed like logp_old (None: the cached log pi_old is dropped and the step evaluates the old policy
        itself -- correct, slower); with old_values also the clipped value loss (self.value_clip)."""
        if old_values is not None and self.value_clip is None:
            raise ValueError("PPO._kl_step: old values were passed but value clipping is off (set_value_clip)")
        self._dispatch_step(s, a, r, adv, rows, logp_old, mean_old, old_values, m_local, m_global)

    def last_grad_norm(self):
        """{"grad_norm", "clip_scale"} of the last step that formed a norm (one readback); zeros before the first one."""
        g = self._need_dev().grad_clip.cpu().numpy()
        return {"grad_norm": float(g[0]), "clip_scale": float(g[1])}

    def set_weights(self, named):
        if self.dev is None:
            self._init_values = {k: np.asarray(v, np.float32) for k, v in named.items()}
        else:
            self.dev.load_params(named)

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        dev = self._need_dev()
        out = dict(dev.export_params())
        out.update(dev.export_old())
        m, v = dev.export_slots()
        for k in m:
            out[k + "/Adam"] = m[k]
            out[k + "/Adam_1"] = v[k]
        out["beta1_power"], out["beta2_power"] = np.float32(self.beta1_power), np.float32(self.beta2_power)
        out["train_step_counter"] = np.int32(self.train_step_counter)
        out["predict_step_counter"] = np.int32(self.predict_step_counter)
        out["episode_counter"] = np.int32(self.episode_counter)
        return out

    def load_state_dict(self, sd):
        dev = self._need_dev()
        old = {k.replace("policy/", "policy_old/", 1): sd.get(k.replace("policy/", "policy_old/", 1), sd[k]) for k in self._variables}
        dev.load_params({k: sd[k] for k in self._variables}, old)
        if all((k + "/Adam") in sd for k in self._variables):
            dev.load_slots({k: sd[k + "/Adam"] for k in self._variables}, {k: sd[k + "/Adam_1"] for k in self._variables})
            self.beta1_power = np.float32(sd.get("beta1_power", ADAM_BETA1))
            self.beta2_power = np.float32(sd.get("beta2_power", ADAM_BETA2))
        self.train_step_counter = int(sd.get("train_step_counter", 0))
        self.predict_step_counter = int(sd.get("predict_step_counter", 0))
        self.episode_counter = int(sd.get("episode_counter", 0))

    def save(self):
        if midist.rank() == 0:
            model_checkpoint = ckpt.save(self.checkpoint_dir, self.episode_counter, self.state_dict())
            print("Model checkpoint saved to {}".format(model_checkpoint))

    def load_latest_checkpoint(self):
        model_checkpoint = ckpt.latest(self.checkpoint_dir)
        if model_checkpoint:
            try:
                self.load_state_dict(ckpt.load(model_checkpoint))
                print("Model checkpoint restored from {}".format(model_checkpoint))
                return True
            except Exception as e:
                print(e)
                return False

    # ------------------------------------------------------------------ training
    def current_learning_rate(self):
        """tf.train.exponential_decay(lr, episode_counter, 1, lr_decay, staircase=True) in fp32 (ppo.py:142)."""
        return np.float32(np.float32(self.learning_rate_value) * np.power(np.float32(self.lr_decay), np.float32(self.episode_counter)))

    def _to_dev(self, a, shape):
        import torch
        a = np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape))      # f64 -> f32 at the feed (ppo.py:108-109)
        return torch.from_numpy(a).to(self.dev.device)

    def _step_resident(self, s, a, r, adv, m_local, m_global, logp_old=None, mean_old=None):
        """One SGD step on device-resident minibatch tensors.  Single rank: one C call (fused forward / losses / backward / Adam, five launches);
        data parallel: gradients, all-reduce, Adam.  logp_old: cached log pi_old(a|s) of these samples (PpoDevice.logp_old), optional.  mean_old: the old policy's
        means of these samples (PpoDevice.old_policy_cache), read with the KL penalty on; without it the penalised step evaluates the old policy itself."""
        self._dispatch_step(s, a, r, adv, None, logp_old, mean_old, None, m_local, m_global)

    def _dispatch_step(self, s, a, r, adv, rows, logp_old, mean_old, old_values, m_local, m_global):
        """The ONE decision behind _step_resident / _step_rows / _kl_step: which device call this minibatch step is.  rows None: contiguous minibatch tensors; else
        the tensors are horizon-batch tables and `rows` (int32 device tensor) names this minibatch.  The switches, the world and the communicator are read once.
          the one-call forms    the KL penalty (train_step_kl), old values (train_step_vclip) and the in-kernel gather (train_step_idx; data parallel train_step_dp
                                with the rows) need MI355_PPO_FUSED / MI355_PPO_IDX (the latter not for the penalised contiguous step) not "0", dev.fused_ok() and, data parallel, the
                                library's communicator.  Without them the first two refuse and plain rows are gathered here into the contiguous forms:
          contiguous, plain     single rank: train_step unless MI355_PPO_FUSED=0 (fused_ok() is not asked: the C entry falls back by itself); a communicator:
                                train_step_dp, one C call; else forward_backward, the all-reduce of the gradient buffer (data parallel), apply_adam."""
        dev, world = self.dev, midist.world_size()
        comm = None if world == 1 else self._dp_comm()
        handle = None if comm is None else comm.handle
        fused, kl = os.environ.get("MI355_PPO_FUSED", "1") != "0", self.kl_penalty is not None
        if self.dual_clip is not None and not (fused and dev.fused_ok()):          # (asked only with the setting on: the per-layer path has no dual clip)
            raise ValueError("PPO: dual clip (PPO.set_dual_clip) exists only in the fused kernels (this policy's shape is outside their range (more than 96 inputs: "
                             "PPO.set_wide_inputs()) or MI355_PPO_FUSED=0)")
        if rows is not None or kl or old_values is not None:
            # (MI355_PPO_IDX is the in-kernel gather's switch; the value-clipped step without the penalty asks it with or without rows, as it always has)
            if not (fused and ((kl and rows is None) or os.environ.get("MI355_PPO_IDX", "1") != "0") and (world == 1 or comm is not None) and dev.fused_ok()):
                if kl or old_values is not None:
                    raise ValueError("%s needs the fused one-call step (this policy's shape is outside the fused kernels' range, MI355_PPO_FUSED=0 / MI355_PPO_IDX=0, "
                                     "or data parallel without the library's communicator)" % ("PPO: the KL penalty" if kl else "PPO._step_rows: value clipping"))
                # (the texts above are pinned word for word by tests/test_ppo_step_dispatch_host.py; more than 96 inputs: PPO.set_wide_inputs(), as rollout.py's say)
                # (shapes outside the fused kernels' range -- e.g. more than 8 actions -- have no in-kernel gather: mi_ppo_fused_shape_ok says so up front and the
                #  rows are gathered here instead; row values themselves are clamped into the tables by the kernels)
                mb = rows.to("cuda" if rows.is_cuda else rows.device).long()
                s, a, r, adv = s[mb].contiguous(), a[mb].contiguous(), r[mb].contiguous(), adv[mb].contiguous()
                logp_old, rows = None if logp_old is None else logp_old[mb].contiguous(), None
        inv_m, gs = 1.0 / m_global, m_local / float(m_global)
        alpha = _adam_alpha(self.current_learning_rate(), self.beta1_power, self.beta2_power)
        if kl:
            if mean_old is None:                               # no table of old means (replay.py): the step evaluates the old policy itself -- correct, slower
                logp_old = None
            dev.train_step_kl(handle, s, a, r, adv, logp_old, mean_old, self.kl_penalty, rows, m_local, inv_m, gs, alpha, ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON,
                              old_values=old_values, clip_range_vf=None if old_values is None else self.value_clip)
        elif old_values is not None:
            dev.train_step_vclip(handle, s, a, r, adv, logp_old, old_values, self.value_clip, rows, m_local, inv_m, gs, alpha, ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON)
        elif rows is not None and world == 1:
            dev.train_step_idx(s, a, r, adv, logp_old, rows, m_local, inv_m, gs, alpha, ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON)
        elif comm is not None:
            # data parallel with the library's communicator live: the step is ONE C call -- the fused chain, the all-reduce of the flat gradient buffer, Adam (round 6);
            # with rows the in-kernel gather is kept: they index THIS rank's tables
            dev.train_step_dp(handle, s, a, r, adv, logp_old, rows, m_local, inv_m, gs, alpha, ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON)
        elif world == 1 and fused:
            dev.train_step(s, a, r, adv, m_local, inv_m, gs, alpha, ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON, logp_old=logp_old)
        else:
            dev.forward_backward(s, a, r, adv, m_local, inv_m, gs)
            if world > 1:
                midist.all_reduce_sum(dev.grads)
            dev.apply_adam(alpha, ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON)
        self.beta1_power = np.float32(self.beta1_power * np.float32(ADAM_BETA1))
        self.beta2_power = np.float32(self.beta2_power * np.float32(ADAM_BETA2))

    def _dp_comm(self):
        """The C-ABI communicator that carries this process's gradient all-reduce inside the one-call data-parallel step (mi_ppo_train_step_dp), or None: single
        rank, torch.distributed as the transport (gloo in the CPU tests, a rank without a usable RCCL), or MI355_DP_HOST_LOOP=1 (the host-sequenced form, A/B runs).
        MI355_DP_SKIP_ALLREDUCE=1 (bench.py only): the recording communicator -- the same C call with its collective recorded instead of issued."""
        if midist.world_size() == 1 or os.environ.get("MI355_DP_HOST_LOOP") == "1":
            return None
        comm = midist.mi_comm()
        if comm is not None and os.environ.get("MI355_DP_SKIP_ALLREDUCE") == "1":
            comm = midist.recording_comm()
        return comm

    def _step_rows(self, s_all, a_all, r_all, adv_all, logp_old_all, rows, m_local, m_global, old_values_all=None):
        """One SGD step on rows `rows` (int32 device tensor) of device-resident horizon-batch tables: the minibatch gather of train.py:199-204 runs inside
        the step's kernels (fused kernels; data parallel: the library's communicator); otherwise the rows are gathered and the contiguous forms take over.
        old_values_all: the table of the values recorded at collection time -- the step clips the value loss with self.value_clip (mi_ppo_train_step_vclip), which only the one-call forms can.  With the KL
        penalty on (set_kl_penalty) the step is _kl_step's without a table of old means.  The decision is _dispatch_step's."""
        if old_values_all is not None and self.value_clip is None:
            raise ValueError("PPO._step_rows: old values were passed but value clipping is off (set_value_clip)")
        # this entry carries no table of the old policy's means (the rollout buffers pass theirs to _kl_step): with the penalty on, the cached log pi_old is dropped and
        # the penalised step evaluates the old policy itself
        self._dispatch_step(s_all, a_all, r_all, adv_all, rows, logp_old_all, None, old_values_all, m_local, m_global)

    def train(self, input_states, taken_actions, returns, advantage):
        """One SGD step on a minibatch + metric update + train_step_counter += 1; returns None (ppo.py:218-229)."""
        if self.value_clip is not None:
            raise ValueError("PPO.train: value clipping is on (set_value_clip) and this call takes no old values: train through a rollout buffer's update(), or "
                             "switch it off with set_value_clip(None)")
        dev = self._need_dev()
        m = len(input_states)
        s = self._to_dev(input_states, (m, self.input_dim))
        a = self._to_dev(taken_actions, (m, self.num_actions))
        r = self._to_dev(returns, (m,))
        adv = self._to_dev(advantage, (m,))
        # data parallel (torch.distributed initialised): every rank passes ITS rows of the global minibatch, equal counts on all ranks;
        # gradients are those of sum_local / M_global and the state-independent entropy term is shared through grad_scale = 1 / world,
        # so that the all-reduced buffer is the gradient of the global mean (mi355/dist.py).  Single process: m_global = m.
        self._step_resident(s, a, r, adv, m, m * midist.world_size())
        if self.train_writer is not None:                      # episodic means (ppo.py:150-163); never on a timed path
            # NO collective here: whether a rank logs is that rank's own business (rank 0 only, usually), and an all-reduce issued by the
            # logging ranks alone would pair with the other ranks' next gradient all-reduce.  A data-parallel rank logs ITS rows' means.
            L = self._local_losses()
            for k, v in zip(("train_loss/policy", "train_loss/value", "train_loss/entropy", "train_loss/loss", "train/prob_ratio"), L):
                self._metric_sums[k] = self._metric_sums.get(k, 0.0) + float(v)
            ta = np.asarray(taken_actions, np.float64).reshape(m, self.num_actions)
            for i in range(self.num_actions):                  # ppo.py:155-158: minibatch means of the taken action, the policy mean and its std
                for tag, val in (("taken_actions", ta[:, i].mean()), ("mean", L[5 + i]), ("std", L[5 + self.num_actions + i])):
                    k = "train_actor/action_{}/{}".format(i, tag)
                    self._metric_sums[k] = self._metric_sums.get(k, 0.0) + float(val)
            self._metric_sums["train/returns"] = self._metric_sums.get("train/returns", 0.0) + float(np.mean(returns))
            self._metric_sums["train/advantage"] = self._metric_sums.get("train/advantage", 0.0) + float(np.mean(advantage))
            self._metric_sums["train/learning_rate"] = self._metric_sums.get("train/learning_rate", 0.0) + float(self.current_learning_rate())
            if self.kl_penalty is not None:
                K = self._local_kl_losses()
                for k, v in (("train/kl", K[0]), ("train_loss/kl_penalty", K[1]), ("train/kl_coef", self.kl_penalty)):
                    self._metric_sums[k] = self._metric_sums.get(k, 0.0) + float(v)
            if self.max_grad_norm is not None:
                g = self.last_grad_norm()
                self._metric_sums["train/grad_norm"] = self._metric_sums.get("train/grad_norm", 0.0) + g["grad_norm"]
                self._metric_sums["train/clip_scale"] = self._metric_sums.get("train/clip_scale", 0.0) + g["clip_scale"]
            self._metric_n += 1
        self.train_step_counter += 1

    def _local_losses(self):
        """Loss scalars + per-action mean / std of the last step from THIS rank's rows, no communication.  The device holds sums over the local
        rows / M_global (so that the gradient all-reduce yields the global mean): times the world size that is the mean over the local rows.
        The entropy term and std = exp(logstd) are state independent -- identical on every rank, left as they are."""
        L = self.dev.losses.clone().cpu().numpy()
        w = midist.world_size()
        if w > 1:
            A = self.num_actions
            L[[0, 1, 4]] *= w
            L[5:5 + A] *= w
            L[3] = -L[0] + L[1] - L[2]
            if self.kl_penalty is not None:
                L[3] += self._local_kl_losses()[1]
        return L

    def _local_kl_losses(self):
        """[mean KL, penalty] of the last penalised step from THIS rank's rows: per-sample means like the policy / value terms (times the world size)."""
        return self.dev.kl_losses.clone().cpu().numpy() * midist.world_size()

    def _global_kl_losses(self):
        """[mean KL, penalty] of the last penalised step; data parallel: summed over the ranks like the other per-sample means (COLLECTIVE)."""
        K = self.dev.kl_losses.clone()
        if midist.world_size() > 1:
            midist.all_reduce_sum(K)
        return K.cpu().numpy()

    def _global_losses(self):
        """The five loss scalars of the last step as numpy.  Data parallel: the device holds this rank's share of the batch means (sums over
        its rows / M_global) for the policy / value terms and the probability ratio; they are summed over the ranks here, the
        state-independent entropy term is already the global value."""
        L = self.dev.losses.clone()
        if midist.world_size() > 1:                            # COLLECTIVE: every rank must call this (train_step() does; train()'s logging does not)
            A = self.num_actions
            keep = L[[2] + list(range(5 + A, 5 + 2 * A))].clone()   # entropy term and std = exp(logstd): identical on every rank, not sums
            midist.all_reduce_sum(L)
            L[[2] + list(range(5 + A, 5 + 2 * A))] = keep
            L[3] = -L[0] + L[1] - L[2]
            if self.kl_penalty is not None:
                L[3] += float(self._global_kl_losses()[1])
        return L.cpu().numpy()

    learn = train                                              # north-star alias

    def train_step(self, input_states, taken_actions, returns, advantage):
        """train() that also returns the five loss scalars {policy, value, entropy, loss, prob_ratio} (for parity tests/benchmarks)."""
        self.train(input_states, taken_actions, returns, advantage)
        L = self._global_losses()
        out = dict(policy_loss=float(L[0]), value_loss=float(L[1]), entropy_loss=float(L[2]), loss=float(L[3]), prob_ratio=float(L[4]))
        if self.kl_penalty is not None:
            K = self._global_kl_losses()
            out["kl"], out["kl_penalty"] = float(K[0]), float(K[1])
        return out

    # ------------------------------------------------------------------ behaviour cloning
    def _clone_kind(self, who, loss):
        """What a clone step refuses without a device: the loss name, and a policy outside the fused kernels' range (there is no per-layer clone step).  -> kind"""
        kind = milib.clone_kind(loss, who)
        kin = (self.input_dim + 7) // 8 * 8
        if not (1 <= self.num_actions <= 8 and kin <= (1024 if self.wide_inputs else 96)) or os.environ.get("MI355_PPO_FUSED", "1") == "0":
            raise ValueError("%s: behaviour cloning exists only in the fused kernels (this policy's shape is outside their range (more than 96 inputs: "
                             "PPO.set_wide_inputs()) or MI355_PPO_FUSED=0)" % who)
        return kind

    def _clone_dispatch(self, kind, s, a_e, r, rows, m_local, m_global, learning_rate=None):
        """One clone step on device tensors: contiguous (rows None) or table rows; single rank or the library's communicator.  Adam's powers advance."""
        dev, world = self.dev, midist.world_size()
        comm = None if world == 1 else self._dp_comm()
        if world > 1 and comm is None:
            raise ValueError("PPO.clone_step: data parallel needs the library's communicator (the clone step is one C call)")
        lr = self.current_learning_rate() if learning_rate is None else np.float32(learning_rate)
        alpha = _adam_alpha(lr, self.beta1_power, self.beta2_power)
        dev.clone_step(None if comm is None else comm.handle, s, a_e, r, kind, rows, m_local, 1.0 / m_global, m_local / float(m_global), alpha,
                       ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON)
        self.beta1_power = np.float32(self.beta1_power * np.float32(ADAM_BETA1))
        self.beta2_power = np.float32(self.beta2_power * np.float32(ADAM_BETA2))

    def clone_step(self, input_states, expert_actions, returns=None, loss="nll", learning_rate=None):
        """One behaviour-cloning SGD step on a minibatch of demonstrations (include/mi355_carla.h, mi_ppo_clone_step): the policy is fitted to the expert's actions
        with loss "nll" (the Gaussian negative log-likelihood: action_logstd learns too) or "mse" (the squared error of the action mean: action_logstd keeps its
        value); with `returns` the value net is fitted to them as in train(), without them it is neither run nor changed.  Like train_step: host arrays in, one
        step, Adam's powers and train_step_counter advance; data parallel, every rank passes its rows.  learning_rate None: current_learning_rate().
        -> {clone_loss, value_loss, loss, mean_sq_error}.  Refused before anything touches a device: an unknown loss, mismatched shapes, expert actions that are
        not finite, and a policy outside the fused kernels' range."""
        kind = self._clone_kind("PPO.clone_step", loss)
        s = np.asarray(input_states, np.float32)
        a_e = np.asarray(expert_actions, np.float32)
        m = s.shape[0] if s.ndim == 2 else 0
        if m < 1 or s.shape != (m, self.input_dim):
            raise ValueError("PPO.clone_step: input_states has shape %s, expected [M, %d] with M >= 1" % (s.shape, self.input_dim))
        if a_e.shape != (m, self.num_actions):
            raise ValueError("PPO.clone_step: expert_actions has shape %s, expected %s" % (a_e.shape, (m, self.num_actions)))
        if not np.isfinite(a_e).all():
            raise ValueError("PPO.clone_step: expert_actions holds values that are not finite")
        if returns is not None:
            returns = np.asarray(returns, np.float32)
            if returns.reshape(-1).shape != (m,):
                raise ValueError("PPO.clone_step: returns has shape %s, expected [%d]" % (returns.shape, m))
        if learning_rate is not None and not (isinstance(learning_rate, (int, float, np.floating)) and not isinstance(learning_rate, bool) and 0 < learning_rate < float("inf")):
            raise ValueError("PPO.clone_step: learning_rate is None or a finite float > 0, got %r" % (learning_rate,))
        self._need_dev()
        self._clone_dispatch(kind, self._to_dev(s, (m, self.input_dim)), self._to_dev(a_e, (m, self.num_actions)),
                             None if returns is None else self._to_dev(returns, (m,)), None, m, m * midist.world_size(), learning_rate)
        self.train_step_counter += 1
        L = self._global_clone_losses()
        return dict(clone_loss=float(L[0]), value_loss=float(L[1]), loss=float(L[3]), mean_sq_error=float(L[4]))

    # ------------------------------------------------------------------ the demonstration term
    def set_demonstration_loss(self, coef, loss="nll"):
        """Keep a supervised term in the PPO objective (DAPG's remedy for a warm start that the first PPO updates undo): loss = L_ppo + coef x clone_loss of a
        minibatch of demonstration rows, formed in the same fused step (include/mi355_carla.h, mi_ppo_train_step_demo; _demo_rows).  coef None switches it off (the
        default), a finite float >= 0 switches it on; loss "nll" or "mse" as in clone_step.  Usable before or after init_session(); bool, str, NaN, inf or a
        negative coefficient and an unknown loss raise ValueError before anything touches a device.  It is no part of a checkpoint."""
        if coef is not None and (isinstance(coef, bool) or not isinstance(coef, (int, float, np.integer, np.floating)) or not (coef >= 0 and coef < float("inf"))):
            raise ValueError("PPO.set_demonstration_loss: the value is None or a finite float >= 0, got %r" % (coef,))
        kind = milib.clone_kind(loss, "PPO.set_demonstration_loss")
        self.demo_coef, self.demo_kind = None if coef is None else float(coef), ("nll", "mse")[kind]

    def _demo_rows(self, s_all, a_all, r_all, adv_all, logp_old_all, mean_old_all, rows, m_local, m_global, demo_s_all, demo_a_all, demo_rows, md_local, md_global,
                   old_values_all=None, coef=None, loss=None):
        """One SGD step with the demonstration term on table rows, next to _step_rows / _kl_step: rows `rows` (int32 device tensor) of the horizon-batch tables and
        rows `demo_rows` of the demonstration tables demo_s_all / demo_a_all, in one fused chain with one Adam update (mi_ppo_train_step_demo).  The KL penalty
        (set_kl_penalty; mean_old_all None: the step evaluates the old policy itself) and value clipping (old_values_all with set_value_clip) apply to the PPO rows.
        There is no per-layer form and no gathered fall-back: a policy outside the fused kernels' range and data parallel without the library's communicator are
        refused by name.  coef / loss: this step's coefficient and loss (the rollout buffers pass their own, decaying coefficient; this object's setting is not
        touched), None: what set_demonstration_loss set.  Adam's powers advance; the counters are the caller's."""
        if coef is None:
            if self.demo_coef is None:
                raise ValueError("PPO._demo_rows: the demonstration term is off (set_demonstration_loss)")
            coef = self.demo_coef
        elif isinstance(coef, bool) or not isinstance(coef, (int, float, np.integer, np.floating)) or not (coef >= 0 and coef < float("inf")):
            raise ValueError("PPO._demo_rows: coef is None or a finite float >= 0, got %r" % (coef,))
        loss = self.demo_kind if loss is None else loss
        if old_values_all is not None and self.value_clip is None:
            raise ValueError("PPO._demo_rows: old values were passed but value clipping is off (set_value_clip)")
        self._clone_kind("PPO._demo_rows", loss)               # (the loss name and the fused range: the same refusal as a clone step's)
        dev, world = self._need_dev(), midist.world_size()
        comm = None if world == 1 else self._dp_comm()
        if world > 1 and comm is None:
            raise ValueError("PPO._demo_rows: data parallel needs the library's communicator (the demonstration step is one C call)")
        if not dev.fused_ok():
            raise ValueError("PPO._demo_rows: the demonstration term exists only in the fused kernels (this policy's shape is outside their range)")
        kl = self.kl_penalty
        if kl is not None and mean_old_all is None:            # no table of old means: the step evaluates the old policy itself -- correct, slower
            logp_old_all = None
        alpha = _adam_alpha(self.current_learning_rate(), self.beta1_power, self.beta2_power)
        dev.train_step_demo(None if comm is None else comm.handle, s_all, a_all, r_all, adv_all, logp_old_all, mean_old_all if kl is not None else None, kl, rows, m_local,
                            demo_s_all, demo_a_all, demo_rows, md_local, loss, coef, 1.0 / md_global, 1.0 / m_global, m_local / float(m_global), alpha,
                            ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON, old_values=old_values_all, clip_range_vf=None if old_values_all is None else self.value_clip)
        self.beta1_power = np.float32(self.beta1_power * np.float32(ADAM_BETA1))
        self.beta2_power = np.float32(self.beta2_power * np.float32(ADAM_BETA2))

    def _clone_rows(self, s_all, a_all, r_all, rows, m_local, m_global, loss="nll", learning_rate=None):
        """One clone step on rows `rows` (int32 device tensor) of device-resident tables states / expert actions / returns (r_all None: policy only): the gather
        runs inside the step's kernels.  Adam's powers advance; the counters are the caller's."""
        kind = self._clone_kind("PPO._clone_rows", loss)
        self._need_dev()
        self._clone_dispatch(kind, s_all, a_all, r_all, rows, m_local, m_global, learning_rate)

    def _global_clone_losses(self):
        """The loss scalars of the last clone step; data parallel: the device holds this rank's share of the batch means, summed here (COLLECTIVE)."""
        L = self.dev.losses[:5].clone()
        if midist.world_size() > 1:
            midist.all_reduce_sum(L)
        return L.cpu().numpy()

    def update_old_policy(self):
        self._need_dev().update_old()

    # ------------------------------------------------------------------ inference
    def predict(self, input_states, greedy=False, write_to_summary=False, noise=None):
        """Returns (action, value); squeezes the batch dim when it is 1 (ppo.py:231-251).  `noise` injects the N(0,1) draw."""
        import torch
        dev = self._need_dev()
        input_states = np.asarray(input_states)
        if len(input_states.shape) != 2:
            input_states = input_states[None] if input_states.ndim == 1 else [input_states]
        s = self._to_dev(input_states, (len(input_states), self.input_dim))
        m = s.shape[0]
        nz = None
        if not greedy:
            if noise is not None:
                nz = self._to_dev(noise, (m, self.num_actions))
            else:
                # exploration noise from the library's own Philox4x32-10 + Box-Muller kernel (mi_normal_philox; the same generator the VAE engine
                # samples with): no torch kernel on the rollout path.  Stream = (seed, rank), offset = values drawn so far.
                nz = torch.empty(m, self.num_actions, device=dev.device)
                n = m * self.num_actions
                milib.get().mi_normal_philox(torch.cuda.current_stream(dev.device).cuda_stream,
                                             0xAC7 + 1000003 * int(self.seed or 0) + midist.rank(), self._noise_offset, milib.ptr(nz), n)
                self._noise_offset += n
        action = torch.empty(m, self.num_actions, device=dev.device)
        value = torch.empty(m, device=dev.device)
        dev.predict(s, m, nz, greedy, action, value)
        sampled_action, value = action.cpu().numpy(), value.cpu().numpy()
        if write_to_summary:
            if self.train_writer is not None:                  # ppo.py:175-180: sampled action, policy mean and std of the FIRST state of the batch
                mean0 = dev.action_mean[0].cpu().numpy()
                o, n = dev.layout["policy/action_logstd"]
                std = np.exp(dev.params[o:o + n].cpu().numpy())
                for i in range(self.num_actions):
                    self.train_writer.add_scalar("predict_actor/action_{}/sampled_action".format(i), sampled_action[0, i], self.predict_step_counter)
                    self.train_writer.add_scalar("predict_actor/action_{}/mean".format(i), float(mean0[i]), self.predict_step_counter)
                    self.train_writer.add_scalar("predict_actor/action_{}/std".format(i), float(std[i]), self.predict_step_counter)
            self.predict_step_counter += 1
        if len(input_states) == 1:
            return sampled_action[0], value[0]
        return sampled_action, value

    def values(self, input_states):
        """V(s) under the current parameters -> float32 [n], without sampling an action.  input_states: host array or device tensor [n, input_dim] (one state
        [input_dim] counts as n = 1; the result is still [1]).  With the fused kernels (PpoDevice.fused_ok()) one forward-only pass of the value net alone
        (mi_ppo_values_idx, in the engine's precision mode, any n); otherwise the value half of predict(greedy=True), whose values it then equals bit for bit."""
        import torch
        dev = self._need_dev()
        if isinstance(input_states, torch.Tensor):
            s = input_states.to(device=dev.device, dtype=torch.float32).reshape(-1, self.input_dim).contiguous()
        else:
            a = np.asarray(input_states)
            s = self._to_dev(a, (1 if a.ndim == 1 else len(a), self.input_dim))
        n = int(s.shape[0])
        if n < 1:
            raise ValueError("PPO.values: no states")
        value = torch.empty(n, device=dev.device)
        if dev.fused_ok():
            dev.values_idx(s, None, n, value)
        else:
            dev.predict(s, n, None, True, torch.empty(n, self.num_actions, device=dev.device), value)
        return value.cpu().numpy()

    def log_probs(self, input_states, taken_actions):
        """log pi_theta(a | s) under the current parameters -> float32 [n].  input_states: host array or device tensor [n, input_dim], taken_actions likewise
        [n, num_actions] (one state / action counts as n = 1; the result is still [1]).  One forward-only pass of the policy net alone (mi_ppo_logp_idx, in the
        engine's precision mode, any n); it needs the fused kernels (PpoDevice.fused_ok()): there is no per-layer form, and without them the call raises."""
        import torch
        dev = self._need_dev()

        def dev_rows(x, width):
            if isinstance(x, torch.Tensor):
                return x.to(device=dev.device, dtype=torch.float32).reshape(-1, width).contiguous()
            a = np.asarray(x)
            return self._to_dev(a, (1 if a.ndim == 1 else len(a), width))
        s = dev_rows(input_states, self.input_dim)
        a = dev_rows(taken_actions, self.num_actions)
        n = int(s.shape[0])
        if n < 1:
            raise ValueError("PPO.log_probs: no states")
        if int(a.shape[0]) != n:
            raise ValueError("PPO.log_probs: %d states and %d actions" % (n, int(a.shape[0])))
        logp = torch.empty(n, device=dev.device)
        dev.logp_idx(s, a, None, n, logp)
        return logp.cpu().numpy()

    def get_episode_idx(self):
        return int(self.episode_counter)

    def get_train_step_idx(self):
        return int(self.train_step_counter)

    def get_predict_step_idx(self):
        return int(self.predict_step_counter)

    # ------------------------------------------------------------------ summaries
    def write_value_to_summary(self, summary_name, value, step):
        if self.train_writer is not None:
            self.train_writer.add_scalar(summary_name, value, step)

    def write_dict_to_summary(self, summary_name, params, step):
        if self.train_writer is not None:                      # the reference adds this summary WITHOUT a global step (ppo.py:269): event step 0
            self.train_writer.add_text(summary_name, {k: str(v) for k, v in params.items()}, 0)

    def write_episodic_summaries(self):
        """Writes the episodic means, then increments episode_counter and resets the accumulators (ppo.py:271-273)."""
        if self.train_writer is not None and self._metric_n:
            for k, v in self._metric_sums.items():
                self.train_writer.add_scalar(k, v / self._metric_n, self.get_episode_idx())
            self.train_writer.flush()
        self.episode_counter += 1
        self._metric_sums, self._metric_n = {}, 0
