"""Device side of the PPO model: HBM buffers (torch tensors as plumbing) + the native engine (csrc/ppo_engine.hip).
No arithmetic here; no CPU fallback."""
import ctypes
from collections import OrderedDict

import numpy as np
import torch

from . import lib as milib
from .init import ppo_variables
from .vae_device import require_gpu


N_STATS = 9                                       # MI_PPO_N_STATS of include/mi355_carla.h


def update_stats_summary(sums):
    """The MI_PPO_N_STATS running sums of mi_ppo_update_stats_idx (count, sum d, sum (r - 1 - d), clipped count, sum r, sum ret, sum ret^2, sum (ret - v),
    sum (ret - v)^2; d = log pi - log pi_old, r = exp(d)) -> the update diagnostics of those samples.  approx_kl is the k3 estimator, mean of r - 1 - log r;
    explained_variance is 1 - Var(ret - v) / Var(ret) with population variances, NaN when Var(ret) is 0.  Host arithmetic in float64; no GPU involved."""
    s = np.asarray(sums, np.float64).reshape(-1)
    if s.shape[0] != N_STATS:
        raise ValueError("update_stats_summary: expected %d sums, got %d" % (N_STATS, s.shape[0]))
    n = float(s[0])
    if not n > 0:
        raise ValueError("update_stats_summary: the sums hold no sample")
    var_ret = s[6] / n - (s[5] / n) ** 2
    var_err = s[8] / n - (s[7] / n) ** 2
    return {"samples": int(round(n)), "approx_kl": float(s[2] / n), "approx_kl_k1": float(-s[1] / n), "clip_fraction": float(s[3] / n), "ratio_mean": float(s[4] / n),
            "value_mse": float(s[8] / n), "explained_variance": float(1.0 - var_err / var_ret) if var_ret > 0 else float("nan")}


N_VCLIP_STATS = 4                                 # MI_PPO_N_VCLIP_STATS of include/mi355_carla.h


def value_clip_summary(sums):
    """The MI_PPO_N_VCLIP_STATS running sums of mi_ppo_value_clip_stats (count, count of |V - V_old| > eps_v, sum of max((V - R)^2, (V_c - R)^2), count of samples
    whose clipped term is the larger one) -> value_clip_fraction, value_loss_clipped (the mean of the clipped objective, not scaled by value_scale, like value_mse)
    and value_grad_zero_fraction (the share of samples the value gradient does not flow from).  Host arithmetic in float64; no GPU involved."""
    s = np.asarray(sums, np.float64).reshape(-1)
    if s.shape[0] != N_VCLIP_STATS:
        raise ValueError("value_clip_summary: expected %d sums, got %d" % (N_VCLIP_STATS, s.shape[0]))
    n = float(s[0])
    if not n > 0:
        raise ValueError("value_clip_summary: the sums hold no sample")
    return {"value_clip_fraction": float(s[1] / n), "value_loss_clipped": float(s[2] / n), "value_grad_zero_fraction": float(s[3] / n)}


N_DUAL_CLIP_STATS = 5                             # MI_PPO_N_DUAL_CLIP_STATS of include/mi355_carla.h


def dual_clip_summary(sums):
    """The MI_PPO_N_DUAL_CLIP_STATS running sums of mi_ppo_dual_clip_stats (count, count of A < 0, count of dual-clipped samples, sum of the dual-clipped surrogate
    s', sum of the plain surrogate s) -> dual_clip_fraction, negative_advantage_fraction, surrogate_mean (the mean of s': minus the policy loss of a step over these
    rows) and surrogate_mean_unclipped (the mean of s).  Host arithmetic in float64; no GPU involved."""
    s = np.asarray(sums, np.float64).reshape(-1)
    if s.shape[0] != N_DUAL_CLIP_STATS:
        raise ValueError("dual_clip_summary: expected %d sums, got %d" % (N_DUAL_CLIP_STATS, s.shape[0]))
    n = float(s[0])
    if not n > 0:
        raise ValueError("dual_clip_summary: the sums hold no sample")
    return {"dual_clip_fraction": float(s[2] / n), "negative_advantage_fraction": float(s[1] / n), "surrogate_mean": float(s[3] / n),
            "surrogate_mean_unclipped": float(s[4] / n)}


N_KL_STATS = 4                                    # MI_PPO_N_KL_STATS of include/mi355_carla.h


def kl_stats_summary(sums):
    """The MI_PPO_N_KL_STATS running sums of mi_ppo_kl_stats_idx (count, sum KL, sum KL^2, sum of the mean part D^2 / (2 sigma^2); KL = the closed-form
    KL(pi_old || pi_theta) per sample) -> {"samples", "kl", "kl_std", "kl_mean_part"}: the mean KL, its population standard deviation over the samples and the
    mean of the part the means contribute (the rest, kl - kl_mean_part, is the state-independent log-std part).  Host arithmetic in float64; no GPU involved."""
    s = np.asarray(sums, np.float64).reshape(-1)
    if s.shape[0] != N_KL_STATS:
        raise ValueError("kl_stats_summary: expected %d sums, got %d" % (N_KL_STATS, s.shape[0]))
    n = float(s[0])
    if not n > 0:
        raise ValueError("kl_stats_summary: the sums hold no sample")
    mean = s[1] / n
    return {"samples": int(round(n)), "kl": float(mean), "kl_std": float(np.sqrt(max(s[2] / n - mean * mean, 0.0))), "kl_mean_part": float(s[3] / n)}


def wide_inputs_mode(mode, who="wide_inputs"):
    """The mode of mi_ppo_set_wide_inputs: False / 0, True / 1 or 2 -> 0, 1 or 2; anything else raises ValueError.  No device and no library involved."""
    if isinstance(mode, bool):
        return int(mode)
    if isinstance(mode, (int, np.integer)) and 0 <= int(mode) <= 2:
        return int(mode)
    raise ValueError("%s: the mode is 0 (fused kernels up to 96 inputs), 1 (up to 1024, K-split layer 1) or 2 (up to 1024, narrow layer 1), got %r" % (who, mode))


class PpoDevice:
    def __init__(self, input_dim, num_actions, action_low, action_high, clip_eps, value_scale, entropy_scale,
                 hidden=(500, 300), max_batch=256, device=None, precision="fp32", wide_inputs=0):
        self.precision = milib.ppo_precision_name(precision)
        self.wide_inputs = wide_inputs_mode(wide_inputs, "PpoDevice")      # mi_ppo_set_wide_inputs: 0 = the fused range ends at 96 inputs (set_wide_inputs)
        require_gpu()
        self.L = milib.get()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.input_dim, self.num_actions, self.hidden = int(input_dim), int(num_actions), tuple(hidden)
        self.clip_eps, self.value_scale, self.entropy_scale = float(clip_eps), float(value_scale), float(entropy_scale)
        self.low = np.ascontiguousarray(np.asarray(action_low, np.float32).reshape(-1))
        self.high = np.ascontiguousarray(np.asarray(action_high, np.float32).reshape(-1))
        self.variables = ppo_variables(self.input_dim, self.num_actions, self.hidden)
        self.kin = (self.input_dim + 7) // 8 * 8
        d = self._desc(1)
        n = self.L.mi_ppo_param_floats(ctypes.byref(d))
        if n <= 0:
            raise milib.MiError("mi_ppo_param_floats: " + self.L.cdll.mi_last_error().decode())
        self.n_flat = int(n)
        cnt = self.L.mi_ppo_tensor_count()
        off, size = np.zeros(cnt, np.int64), np.zeros(cnt, np.int64)
        self.L.mi_ppo_param_layout(ctypes.byref(d), off.ctypes.data, size.ctypes.data, cnt)
        self.layout = OrderedDict((name, (int(o), int(s))) for name, o, s in zip(self.variables, off, size))
        z = lambda: torch.zeros(self.n_flat, device=self.device)   # noqa: E731
        self.params, self.params_old, self.grads, self.adam_m, self.adam_v = z(), z(), z(), z(), z()
        self.handle = None
        self.max_batch = 0
        self.max_grad_norm = None                     # global-norm gradient clipping (set_max_grad_norm); None: off
        self.dual_clip = None                         # dual-clip PPO (set_dual_clip); None: off
        self._create(max_batch)

    def _desc(self, max_batch):
        return milib.MiPpoDesc(int(max_batch), self.input_dim, self.num_actions, self.hidden[0], self.hidden[1],
                               self.clip_eps, self.value_scale, self.entropy_scale)

    def _create(self, max_batch):
        # the new engine is created while the old one still exists, and the old one is destroyed behind it: freed first, the C side's allocator hands the same
        # address out again unless something else took it in between, so whether `handle` changed across ensure_batch() depended on the heap's state
        # (tests/test_q_grad_clip_gpu.py::test_setting_survives_ensure_batch tells a recreated engine by it).  Both engines share the parameter buffers; the
        # two workspaces coexist for this call only
        old = self.handle
        d = self._desc(max_batch)
        nbytes = int(self.L.mi_ppo_workspace_bytes(ctypes.byref(d)))
        self.workspace = torch.empty(nbytes, device=self.device, dtype=torch.uint8)
        p = milib.ptr
        self.handle = self.L.mi_ppo_create(ctypes.byref(d), p(self.params), p(self.params_old), p(self.grads), p(self.adam_m), p(self.adam_v),
                                           p(self.workspace), nbytes, self.low.ctypes.data, self.high.ctypes.data)
        if old is not None:
            self.L.mi_ppo_destroy(old)
        if not self.handle:
            raise milib.MiError("mi_ppo_create: " + self.L.cdll.mi_last_error().decode())
        # a new engine starts in fp32 and with the narrow fused range: both modes are applied to every engine this object creates (ensure_batch recreates it for
        # larger batches), the range first -- it decides whether the split mode has kernels
        try:
            self.L.mi_ppo_set_wide_inputs(self.handle, self.wide_inputs)
            self.L.mi_ppo_set_precision(self.handle, milib.PPO_PRECISIONS[self.precision])      # raises MiError (no fp32 fallback) where the mode has no kernels
        except milib.MiError:
            self.L.mi_ppo_destroy(self.handle)
            self.handle = None
            raise
        self.max_batch = int(max_batch)
        addr = self.L.mi_ppo_buffer(self.handle, 0)
        o = addr - self.workspace.data_ptr()
        # [policy, value, entropy, total, mean prob ratio, mean action_mean[A], std[A]] of the last minibatch step
        self.losses = self.workspace[o:o + 4 * (5 + 2 * self.num_actions)].view(torch.float32)
        # [mean KL(pi_old || pi), beta x mean KL] of the last train_step_kl: the two floats behind `losses` (no other step writes them)
        self.kl_losses = self.workspace[o + 4 * (5 + 2 * self.num_actions):o + 4 * (7 + 2 * self.num_actions)].view(torch.float32)
        addr = self.L.mi_ppo_buffer(self.handle, 1)
        o = addr - self.workspace.data_ptr()
        self.action_mean = self.workspace[o:o + 4 * int(max_batch) * self.num_actions].view(torch.float32).view(int(max_batch), self.num_actions)
        addr = self.L.mi_ppo_buffer(self.handle, 2)
        o = addr - self.workspace.data_ptr()
        # [gradient norm, clip factor, the limit, 0] of the last norm the engine formed (a clipped step, or grad_norm())
        self.grad_clip = self.workspace[o:o + 16].view(torch.float32)
        addr = self.L.mi_ppo_buffer(self.handle, 3)
        o = addr - self.workspace.data_ptr()
        # d loss / d value-head output per sample of the last step (the step's workspace; exactly 0 where value clipping stops the gradient)
        self.value_head_grad = self.workspace[o:o + 4 * int(max_batch)].view(torch.float32)
        addr = self.L.mi_ppo_buffer(self.handle, 4)
        o = addr - self.workspace.data_ptr()
        # [demo_loss, demo_coef x demo_loss, mean_sq_error] of the last train_step_demo (no other step writes them)
        self.demo_losses = self.workspace[o:o + 12].view(torch.float32)
        addr = self.L.mi_ppo_buffer(self.handle, 5)
        o = addr - self.workspace.data_ptr()
        # d loss / d action-mean head output per sample of the last step (the step's workspace; exactly 0 on a dual-clipped sample with the KL penalty off)
        self.policy_head_grad = self.workspace[o:o + 4 * int(max_batch) * self.num_actions].view(torch.float32).view(int(max_batch), self.num_actions)
        # like the precision, the clipping limit is applied to every engine this object creates
        self.L.mi_ppo_set_max_grad_norm(self.handle, 0.0 if self.max_grad_norm is None else self.max_grad_norm)
        # ... and the dual-clip constant (the loss coefficients travel in the descriptor, which _desc fills from the live attributes)
        self.L.mi_ppo_set_dual_clip(self.handle, 0.0 if self.dual_clip is None else self.dual_clip)

    def ensure_batch(self, m):
        if m > self.max_batch:
            torch.cuda.synchronize(self.device)
            self._create(max(m, 2 * self.max_batch))

    def close(self):
        if self.handle is not None:
            self.L.mi_ppo_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    # ---- TF-named variables <-> flat layout (first-layer kernels are zero-padded from input_dim to kin rows) ----
    def _to_flat(self, named, scope="policy"):
        flat = np.zeros(self.n_flat, np.float32)
        for name, (o, s) in self.layout.items():
            a = np.asarray(named[name.replace("policy/", scope + "/", 1)], np.float32)
            if tuple(a.shape) != tuple(self.variables[name]):
                raise ValueError("%s: shape %s, expected %s" % (name, a.shape, self.variables[name]))
            if name.endswith(("dense/kernel", "dense_2/kernel")):
                pad = np.zeros((self.kin, a.shape[1]), np.float32)
                pad[:a.shape[0]] = a
                a = pad
            flat[o:o + s] = a.reshape(-1)
        return flat

    def _from_flat(self, flat, scope="policy"):
        out = OrderedDict()
        for name, shape in self.variables.items():
            o, s = self.layout[name]
            if name.endswith(("dense/kernel", "dense_2/kernel")):
                a = flat[o:o + s].reshape(self.kin, shape[1])[:shape[0]].copy()
            else:
                a = flat[o:o + s].reshape(shape).copy()
            out[name.replace("policy/", scope + "/", 1)] = a
        return out

    def load_params(self, named, old_named=None):
        self.params.copy_(torch.from_numpy(self._to_flat(named)))
        if old_named is not None:
            self.params_old.copy_(torch.from_numpy(self._to_flat(old_named, "policy_old")))

    def load_slots(self, m_named, v_named):
        self.adam_m.copy_(torch.from_numpy(self._to_flat(m_named)))
        self.adam_v.copy_(torch.from_numpy(self._to_flat(v_named)))

    def export_params(self):
        return self._from_flat(self.params.cpu().numpy())

    def export_old(self):
        return self._from_flat(self.params_old.cpu().numpy(), "policy_old")

    def export_slots(self):
        return self._from_flat(self.adam_m.cpu().numpy()), self._from_flat(self.adam_v.cpu().numpy())

    def export_grads(self):
        return self._from_flat(self.grads.cpu().numpy())

    # ---- steps ----
    def update_old(self):
        self.L.mi_ppo_update_old(self.handle, self.stream())

    def predict(self, states, M, noise, greedy, action, value):
        self.ensure_batch(M)
        p = milib.ptr
        self.L.mi_ppo_predict(self.handle, self.stream(), p(states), int(M), p(noise), int(greedy), p(action), p(value))

    def forward_backward(self, states, actions, returns, advantage, M, inv_m, grad_scale):
        self.ensure_batch(M)
        p = milib.ptr
        self.L.mi_ppo_forward_backward(self.handle, self.stream(), p(states), p(actions), p(returns), p(advantage), int(M), float(inv_m), float(grad_scale))

    def train_step(self, states, actions, returns, advantage, M, inv_m, grad_scale, alpha, beta1=0.9, beta2=0.999, epsilon=1e-8, logp_old=None):
        """The whole minibatch step in one C call (single rank): fused forward / losses / backward / Adam (csrc/ppo_fused.hip)."""
        self.ensure_batch(M)
        p = milib.ptr
        self.L.mi_ppo_train_step(self.handle, self.stream(), p(states), p(actions), p(returns), p(advantage), p(logp_old), int(M), float(inv_m), float(grad_scale),
                                 float(alpha), float(beta1), float(beta2), float(epsilon))

    def train_step_idx(self, states, actions, returns, advantage, logp_old, row_idx, M, inv_m, grad_scale, alpha, beta1=0.9, beta2=0.999, epsilon=1e-8):
        """train_step on rows `row_idx` (int32 device tensor [M]) of the horizon-batch tables: the gather happens inside the kernels."""
        self.ensure_batch(M)
        p = milib.ptr
        self.L.mi_ppo_train_step_idx(self.handle, self.stream(), p(states), p(actions), p(returns), p(advantage), p(logp_old), p(row_idx), int(states.shape[0]), int(M),
                                     float(inv_m), float(grad_scale), float(alpha), float(beta1), float(beta2), float(epsilon))

    def train_step_dp(self, comm_handle, states, actions, returns, advantage, logp_old, row_idx, M, inv_m, grad_scale, alpha, beta1=0.9, beta2=0.999, epsilon=1e-8):
        """One DATA-PARALLEL minibatch step in one C call (mi_ppo_train_step_dp, round 6): the fused chain on this rank's M rows, one all-reduce of the flat gradient
        buffer through the library communicator, Adam.  row_idx (int32 device tensor [M]) names rows of the horizon-batch tables (gather inside the kernels) or is None
        (contiguous minibatch tensors)."""
        self.ensure_batch(M)
        p = milib.ptr
        self.L.mi_ppo_train_step_dp(self.handle, comm_handle, self.stream(), p(states), p(actions), p(returns), p(advantage), p(logp_old), p(row_idx),
                                    int(states.shape[0]), int(M), float(inv_m), float(grad_scale), float(alpha), float(beta1), float(beta2), float(epsilon))

    def train_step_vclip(self, comm_handle, states, actions, returns, advantage, logp_old, old_values, clip_range_vf, row_idx, M, inv_m, grad_scale, alpha,
                         beta1=0.9, beta2=0.999, epsilon=1e-8, adam=True):
        """The minibatch step with PPO2-style value-function clipping (mi_ppo_train_step_vclip): the value term is max((V - R)^2, (V_c - R)^2) with V_c = V clamped
        into old_values +- clip_range_vf (a positive float or inf).  One entry for the three forms: row_idx None (contiguous minibatch tensors, as train_step) or an
        int32 device tensor [M] naming rows of the horizon-batch tables, old_values among them (as train_step_idx); comm_handle None or a communicator (as
        train_step_dp).  adam False: stops with the gradients in the flat buffer (forward_backward's role)."""
        self.ensure_batch(M)
        p = milib.ptr
        self.L.mi_ppo_train_step_vclip(self.handle, comm_handle, self.stream(), p(states), p(actions), p(returns), p(advantage), p(logp_old), p(old_values),
                                       float(clip_range_vf), p(row_idx), int(states.shape[0]), int(M), float(inv_m), float(grad_scale), 1 if adam else 0,
                                       float(alpha), float(beta1), float(beta2), float(epsilon))

    def old_policy_cache(self, states, actions, M, logp_out, mean_out):
        """logp_old() that keeps the old policy's action means as well (mi_ppo_old_policy_cache): logp_out [M] (bit for bit logp_old's), mean_out [M, A] -- the two
        tables train_step_kl and kl_stats read."""
        self.ensure_batch(M)
        p = milib.ptr
        self.L.mi_ppo_old_policy_cache(self.handle, self.stream(), p(states), p(actions), int(M), p(logp_out), p(mean_out))

    def train_step_kl(self, comm_handle, states, actions, returns, advantage, logp_old, mean_old, kl_coef, row_idx, M, inv_m, grad_scale, alpha,
                      beta1=0.9, beta2=0.999, epsilon=1e-8, adam=True, old_values=None, clip_range_vf=None):
        """The minibatch step with the KL penalty kl_coef x mean KL(pi_old || pi_theta) added to the clipped surrogate (mi_ppo_train_step_kl; kl_coef a finite float
        >= 0, 0 measures only).  logp_old / mean_old: the tables old_policy_cache filled, or both None (the step evaluates the old policy itself).  One entry for
        every form, as train_step_vclip: row_idx None or an int32 device tensor [M] naming rows of the tables; comm_handle None or a communicator; adam False stops
        with the gradients in the flat buffer; old_values / clip_range_vf: the clipped value loss of train_step_vclip on top.  `kl_losses` holds [mean KL, penalty]."""
        self.ensure_batch(M)
        p = milib.ptr
        self.L.mi_ppo_train_step_kl(self.handle, comm_handle, self.stream(), p(states), p(actions), p(returns), p(advantage), p(logp_old), p(mean_old), float(kl_coef),
                                    p(old_values), 0.0 if old_values is None else float(clip_range_vf), p(row_idx), int(states.shape[0]), int(M), float(inv_m),
                                    float(grad_scale), 1 if adam else 0, float(alpha), float(beta1), float(beta2), float(epsilon))

    def clone_step(self, comm_handle, states, expert_actions, returns, kind, row_idx, M, inv_m, grad_scale, alpha,
                   beta1=0.9, beta2=0.999, epsilon=1e-8, adam=True):
        """One behaviour-cloning step (mi_ppo_clone_step): the policy is fitted to the expert's actions -- kind "nll" (the Gaussian negative log-likelihood, logstd
        learns too) or "mse" (the squared error of the action mean, logstd gets a gradient of exactly 0) -- and, with `returns`, the value net to them; returns None
        is the policy-only form, which neither runs nor touches the value net.  One entry for every form, as train_step_kl: row_idx None or an int32 device tensor
        [M] naming rows of the tables states / expert_actions / returns; comm_handle None or a communicator; adam False stops with the gradients in the flat buffer.
        `losses` then holds [clone_loss, value_loss, 0, loss, mean_sq_error] (clone_losses() reads them)."""
        kind = milib.clone_kind(kind, "PpoDevice.clone_step")
        self.ensure_batch(M)
        p = milib.ptr
        self.L.mi_ppo_clone_step(self.handle, comm_handle, self.stream(), p(states), p(expert_actions), p(returns), kind, p(row_idx), int(states.shape[0]), int(M),
                                 float(inv_m), float(grad_scale), 1 if adam else 0, float(alpha), float(beta1), float(beta2), float(epsilon))

    def train_step_demo(self, comm_handle, states, actions, returns, advantage, logp_old, mean_old, kl_coef, row_idx, M, demo_states, demo_actions, demo_row_idx,
                        M_demo, demo_kind, demo_coef, inv_m_demo, inv_m, grad_scale, alpha, beta1=0.9, beta2=0.999, epsilon=1e-8, adam=True,
                        old_values=None, clip_range_vf=None):
        """The PPO step with a demonstration term (mi_ppo_train_step_demo): M PPO rows and M_demo demonstration rows in one fused chain, one gradient, one Adam
        update; loss = L_ppo + demo_coef x clone_loss(demonstration rows), demo_kind "nll" / "mse", policy only.  The PPO side as train_step_kl -- kl_coef None: no
        KL penalty (mean_old is not read); old_values / clip_range_vf: the clipped value loss; row_idx None or an int32 device tensor [M] naming rows of the PPO
        tables -- and the demonstration side likewise: demo_row_idx None (demo_states / demo_actions contiguous) or rows of the demonstration tables.  comm_handle
        None or a communicator; adam False stops with the gradients in the flat buffer.  `demo_losses` holds [demo_loss, demo_coef x demo_loss, mean_sq_error]."""
        demo_kind = milib.clone_kind(demo_kind, "PpoDevice.train_step_demo")
        self.ensure_batch(int(M) + int(M_demo))
        p = milib.ptr
        self.L.mi_ppo_train_step_demo(self.handle, comm_handle, self.stream(), p(states), p(actions), p(returns), p(advantage), p(logp_old), p(mean_old),
                                      0 if kl_coef is None else 1, 0.0 if kl_coef is None else float(kl_coef), p(old_values),
                                      0.0 if old_values is None else float(clip_range_vf), p(row_idx), int(states.shape[0]), int(M), p(demo_states), p(demo_actions),
                                      p(demo_row_idx), int(demo_states.shape[0]), int(M_demo), demo_kind, float(demo_coef), float(inv_m_demo), float(inv_m),
                                      float(grad_scale), 1 if adam else 0, float(alpha), float(beta1), float(beta2), float(epsilon))

    def clone_losses(self):
        """{clone_loss, value_loss, loss, mean_sq_error} of the last clone_step (one readback)."""
        L = self.losses[:5].cpu().numpy()
        return {"clone_loss": float(L[0]), "value_loss": float(L[1]), "loss": float(L[3]), "mean_sq_error": float(L[4])}

    def kl_stats(self, states, mean_old, row_idx, M, stats, scratch, accumulate=False):
        """The N_KL_STATS sums of the exact KL(pi_old || pi_theta) (mi_ppo_kl_stats_idx; kl_stats_summary turns them into a dict) over rows `row_idx` (int32 device
        tensor [M]) of the tables states / mean_old under the CURRENT parameters, into `stats` (float64 device tensor [N_KL_STATS]; accumulate: added to it).
        scratch: float64 device tensor of kl_stats_scratch_doubles(M) entries.  Forward only: nothing of the training state is written."""
        self.ensure_batch(M)
        p = milib.ptr
        self.L.mi_ppo_kl_stats_idx(self.handle, self.stream(), p(states), p(mean_old), p(row_idx), int(states.shape[0]), int(M), 1 if accumulate else 0, p(scratch), p(stats))

    def kl_stats_scratch_doubles(self, M):
        return int(self.L.mi_ppo_kl_stats_scratch_doubles(int(M)))

    def value_clip_stats(self, values_new, old_values, returns, row_idx, M, clip_range_vf, stats, scratch, accumulate=False):
        """The N_VCLIP_STATS sums of the value-clipping diagnostics (mi_ppo_value_clip_stats; value_clip_summary turns them into a dict) over rows `row_idx` (int32
        device tensor [M]) of the tables values_new (the value_out table update_stats fills) / old_values / returns, into `stats` (float64 device tensor
        [N_VCLIP_STATS]; accumulate: added to it).  scratch: float64 device tensor of value_clip_scratch_doubles(M) entries.  Needs no engine."""
        p = milib.ptr
        self.L.mi_ppo_value_clip_stats(self.stream(), p(values_new), p(old_values), p(returns), p(row_idx), int(values_new.shape[0]), int(M), float(clip_range_vf),
                                       1 if accumulate else 0, p(scratch), p(stats))

    def value_clip_scratch_doubles(self, M):
        return int(self.L.mi_ppo_value_clip_stats_scratch_doubles(int(M)))

    def engine_precision(self):
        """The engine's own record of its mode (mi_ppo_precision): MI_F32 or MI_BF16X3."""
        return int(self.L.cdll.mi_ppo_precision(self.handle))      # (the raw call: a mode is a non-zero return, not an error)

    def set_precision(self, precision):
        """The precision of the training forms (mi_ppo_set_precision): "fp32" or "bf16x3".  MiError where the split mode has no kernels (an engine on the per-layer
        path); the mode is then unchanged.  Kept across ensure_batch."""
        name = milib.ppo_precision_name(precision)
        self.L.mi_ppo_set_precision(self.handle, milib.PPO_PRECISIONS[name])
        self.precision = name

    def set_wide_inputs(self, mode):
        """Which input widths the fused kernels take (mi_ppo_set_wide_inputs): 0 (the default) up to 96 padded inputs; 1 up to 1024, layer 1 of a wide policy through
        the K-split kernel; 2 up to 1024 with the narrow layer-1 kernel at every width (kept for measuring 1 against).  Routing only: parameters and optimiser state
        are laid out the same on every path, so it may change between two steps.  Kept across ensure_batch."""
        mode = wide_inputs_mode(mode, "PpoDevice.set_wide_inputs")
        self.L.mi_ppo_set_wide_inputs(self.handle, mode)
        self.wide_inputs = mode

    def engine_wide_inputs(self):
        """The engine's own record of the mode (mi_ppo_wide_inputs)."""
        return int(self.L.cdll.mi_ppo_wide_inputs(self.handle))      # (the raw call: a mode is a non-zero return, not an error)

    def fused_ok(self):
        """True when the fused kernels (in-kernel minibatch gather, cached log pi_old) take this engine's shape; else only the per-layer path runs."""
        return bool(self.L.mi_ppo_fused_shape_ok(self.handle))

    def logp_old(self, states, actions, M, out):
        """log pi_old(a | s) of M samples under theta_old (computed once per horizon batch; theta_old only changes in update_old())."""
        self.ensure_batch(M)
        p = milib.ptr
        self.L.mi_ppo_logp_old(self.handle, self.stream(), p(states), p(actions), int(M), p(out))

    def update_stats(self, states, actions, returns, logp_old, row_idx, M, stats, scratch, accumulate=False, logp_new_out=None, value_out=None):
        """The N_STATS sums of the update diagnostics (mi_ppo_update_stats_idx; update_stats_summary turns them into a dict) over rows `row_idx` (int32 device tensor
        [M]) of the horizon-batch tables under the CURRENT parameters, into `stats` (float64 device tensor [N_STATS]; accumulate: added to it).  scratch: float64
        device tensor of stats_scratch_doubles(M) entries.  logp_new_out / value_out: float32 tables of states.shape[0] entries, written at the named rows only.
        Forward only: parameters, optimiser state, gradients and the losses buffer keep their contents."""
        self.ensure_batch(M)
        p = milib.ptr
        self.L.mi_ppo_update_stats_idx(self.handle, self.stream(), p(states), p(actions), p(returns), p(logp_old), p(row_idx), int(states.shape[0]), int(M),
                                       1 if accumulate else 0, p(scratch), p(stats), p(logp_new_out), p(value_out))

    def values_idx(self, states, row_idx, M, out):
        """V(s) under the CURRENT parameters of M rows of the table `states` [n_rows, input_dim] (mi_ppo_values_idx): the value net alone, forward only.  row_idx: an
        int32 device tensor [M] naming table rows, or None (rows 0 .. M-1).  The value of a row goes to the entry of `out` (float32 device tensor, n_rows entries) with
        that row's number; a row outside [0, n_rows) stores nothing, and entries no row names keep their contents.  M may exceed max_batch: the entry walks the chunks
        itself and the engine is NOT grown.  Bit for bit the value_out table of update_stats.  Nothing of the training state is written."""
        if int(out.shape[0]) < int(states.shape[0]):
            raise ValueError("PpoDevice.values_idx: `out` has %d entries for a table of %d rows" % (int(out.shape[0]), int(states.shape[0])))
        p = milib.ptr
        self.L.mi_ppo_values_idx(self.handle, self.stream(), p(states), p(row_idx), int(states.shape[0]), int(M), p(out))

    def logp_idx(self, states, actions, row_idx, M, out):
        """log pi_theta(a | s) under the CURRENT parameters of M rows of the tables `states` [n_rows, input_dim] / `actions` [n_rows, num_actions]
        (mi_ppo_logp_idx): the policy net alone, forward only -- the twin of values_idx.  row_idx: an int32 device tensor [M] naming table rows, or None (rows
        0 .. M-1).  The result of a row goes to the entry of `out` (float32 device tensor, n_rows entries) with that row's number; a row outside [0, n_rows) stores
        nothing, and entries no row names keep their contents.  M may exceed max_batch: the entry walks the chunks itself and the engine is NOT grown.  Bit for
        bit the logp_new_out table of update_stats, and right behind update_old_policy() the cache of logp_old.  Nothing of the training state is written."""
        if int(out.shape[0]) < int(states.shape[0]):
            raise ValueError("PpoDevice.logp_idx: `out` has %d entries for a table of %d rows" % (int(out.shape[0]), int(states.shape[0])))
        if int(actions.shape[0]) < int(states.shape[0]):
            raise ValueError("PpoDevice.logp_idx: `actions` has %d rows for a table of %d rows" % (int(actions.shape[0]), int(states.shape[0])))
        p = milib.ptr
        self.L.mi_ppo_logp_idx(self.handle, self.stream(), p(states), p(actions), p(row_idx), int(states.shape[0]), int(M), p(out))

    def stats_scratch_doubles(self, M):
        return int(self.L.mi_ppo_update_stats_scratch_doubles(int(M)))

    def set_max_grad_norm(self, max_norm):
        """Global-norm gradient clipping in front of Adam (mi_ppo_set_max_grad_norm): None switches it off, a positive float (inf: measure only) switches it on for
        apply_adam and every train_step form.  Kept across ensure_batch."""
        self.max_grad_norm = milib.max_grad_norm_value(max_norm, "PpoDevice.set_max_grad_norm")
        self.L.mi_ppo_set_max_grad_norm(self.handle, 0.0 if self.max_grad_norm is None else self.max_grad_norm)

    def set_dual_clip(self, c):
        """Dual-clip PPO (mi_ppo_set_dual_clip): None switches it off, a float > 1 (inf: on, and no sample is ever dual-clipped) switches it on for every fused
        step form -- a sample with A < 0 whose c A lies above the clipped surrogate takes c A and gives the policy no gradient.  Kept across ensure_batch."""
        self.dual_clip = milib.dual_clip_value(c, "PpoDevice.set_dual_clip")
        self.L.mi_ppo_set_dual_clip(self.handle, 0.0 if self.dual_clip is None else self.dual_clip)

    def engine_dual_clip(self):
        """The engine's own record of the constant (mi_ppo_dual_clip): 0.0 = off."""
        return float(self.L.mi_ppo_dual_clip(self.handle))

    def set_loss_coefs(self, clip_eps, value_scale, entropy_scale):
        """Replace the three loss coefficients on the live engine (mi_ppo_set_loss_coefs): clip_eps finite and > 0, value_scale and entropy_scale finite and >= 0;
        ValueError otherwise, nothing changed.  Every later call reads them: the steps, update_stats' clipped fraction, the per-layer path.  Parameters and optimiser
        state stay.  Kept across ensure_batch (the next engine's descriptor is filled from them)."""
        ce, vs, es = milib.loss_coef_values(clip_eps, value_scale, entropy_scale, "PpoDevice.set_loss_coefs")
        self.L.mi_ppo_set_loss_coefs(self.handle, ce, vs, es)
        self.clip_eps, self.value_scale, self.entropy_scale = ce, vs, es

    def engine_loss_coefs(self):
        """The engine's own record of (clip_eps, value_scale, entropy_scale) (mi_ppo_loss_coefs)."""
        out = (ctypes.c_float * 3)()
        base = ctypes.addressof(out)
        self.L.mi_ppo_loss_coefs(self.handle, base, base + 4, base + 8)
        return float(out[0]), float(out[1]), float(out[2])

    def dual_clip_stats(self, logp_new, logp_old, advantage, row_idx, M, clip_eps, dual_clip, stats, scratch, accumulate=False):
        """The N_DUAL_CLIP_STATS sums of the dual-clip diagnostics (mi_ppo_dual_clip_stats; dual_clip_summary turns them into a dict) over rows `row_idx` (int32
        device tensor [M]) of the tables logp_new (the logp_new_out table update_stats fills) / logp_old / advantage, into `stats` (float64 device tensor
        [N_DUAL_CLIP_STATS]; accumulate: added to it).  scratch: float64 device tensor of dual_clip_scratch_doubles(M) entries.  Needs no engine."""
        p = milib.ptr
        self.L.mi_ppo_dual_clip_stats(self.stream(), p(logp_new), p(logp_old), p(advantage), p(row_idx), int(logp_new.shape[0]), int(M), float(clip_eps),
                                      float(dual_clip), 1 if accumulate else 0, p(scratch), p(stats))

    def dual_clip_scratch_doubles(self, M):
        return int(self.L.mi_ppo_dual_clip_stats_scratch_doubles(int(M)))

    def engine_max_grad_norm(self):
        """The engine's own record of the limit (mi_ppo_max_grad_norm): 0.0 = off."""
        return float(self.L.mi_ppo_max_grad_norm(self.handle))

    def grad_norm(self, max_norm):
        """The global L2 norm of the gradient buffer as it stands (e.g. behind forward_backward) and the factor a limit of max_norm (a positive float or inf) gives,
        into `grad_clip` ([norm, scale, max_norm, 0], device).  Nothing else is written: parameters, optimiser state and gradients keep their contents."""
        self.L.mi_ppo_grad_norm(self.handle, self.stream(), float(max_norm))

    def apply_adam(self, alpha, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.L.mi_ppo_apply_adam(self.handle, self.stream(), float(alpha), float(beta1), float(beta2), float(epsilon))
