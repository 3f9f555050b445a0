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
"""
import os

import numpy as np

from mi355 import lib as milib


class RolloutStep:
    def __init__(self, vae, ppo, seed=None, io=None):
        import torch
        self.vae, self.ppo = vae, ppo
        vdev, pdev = vae._need_dev(), ppo._need_dev()
        self.L = vdev.L
        self.device = vdev.device
        self.z_dim, self.A = int(vae.z_dim), int(ppo.num_actions)
        self.n_meas = int(ppo.input_dim) - self.z_dim
        if self.n_meas < 0:
            raise ValueError("the policy takes fewer inputs than the VAE's latent size")
        self.frame_bytes = int(np.prod(vdev.source_shape))
        self._noise_off = (self.frame_bytes + 15) // 16 * 16                         # float region: measurements, then noise
        nbytes = self._noise_off + 4 * (self.n_meas + self.A)
        self.h_in = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.d_in = None                                                             # (allocated below for io="device")
        self.h_out = torch.empty(self.A + 1 + self.z_dim, dtype=torch.float32).pin_memory()
        self.io = io or os.environ.get("MI355_ROLLOUT_IO", "pinned")
        if self.io not in ("pinned", "device"):
            raise ValueError("RolloutStep: io must be 'pinned' or 'device'")
        self.d_out = torch.empty(self.A + 1 + self.z_dim, dtype=torch.float32, device=self.device) if self.io == "device" else None
        self.d_in = torch.empty(nbytes, dtype=torch.uint8, device=self.device) if self.io == "device" else None
        self._in_np = self.h_in.numpy()
        self._f_np = self._in_np[self._noise_off:].view(np.float32)
        self._out_np = self.h_out.numpy()
        self._rng = np.random.Generator(np.random.Philox(int(seed if seed is not None else (ppo.seed or 0)) + 0xAC7))

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


MAX_ENVS = 1024                                                                      # MI_ROLLOUT_MAX_ENVS of include/mi355_carla.h


class BatchedRolloutStep:
    """RolloutStep for up to `num_envs` environments per call (mi_rollout_step_batch): frames_u8 [n, H, W, 3] uint8 and measurements [n, k] in,
    (actions float32 [n, A], values float32 [n], states float64 [n, z_dim + k]) out, 1 <= n <= num_envs -- environments finish their episodes at
    different times.  Row e is what RolloutStep gives for frame e: np.append(vae.encode([frame_e])[0], meas_e) and model.predict of it."""

    def __init__(self, vae, ppo, num_envs, seed=None, io=None):
        import torch
        self.vae, self.ppo = vae, ppo
        self.num_envs = int(num_envs)
        if not 1 <= self.num_envs <= MAX_ENVS:
            raise ValueError("BatchedRolloutStep: 1 <= num_envs <= %d" % MAX_ENVS)
        vdev, pdev = vae._need_dev(), ppo._need_dev()
        self.L = vdev.L
        self.device = vdev.device
        self.z_dim, self.A = int(vae.z_dim), int(ppo.num_actions)
        self.n_meas = int(ppo.input_dim) - self.z_dim
        if self.n_meas < 0:
            raise ValueError("the policy takes fewer inputs than the VAE's latent size")
        self.io = io or os.environ.get("MI355_ROLLOUT_IO", "pinned")
        if self.io not in ("pinned", "device"):
            raise ValueError("BatchedRolloutStep: io must be 'pinned' or 'device'")
        pdev.ensure_batch(self.num_envs)                                             # recreates the engine when it grows: ppo.dev.handle is read per call
        E, self.row = self.num_envs, self.A + 1 + self.z_dim
        self.frame_bytes = int(np.prod(vdev.source_shape))
        self._f_off = (E * self.frame_bytes + 15) // 16 * 16                         # float region: measurements [E, k], then noise [E, A]
        nbytes = self._f_off + 4 * E * (self.n_meas + self.A)
        self.h_in = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.h_out = torch.empty(E * self.row, dtype=torch.float32).pin_memory()
        dev_io = self.io == "device"
        self.d_in = torch.empty(nbytes, dtype=torch.uint8, device=self.device) if dev_io else None
        self.d_out = torch.empty(E * self.row, dtype=torch.float32, device=self.device) if dev_io else None
        self.scratch_bytes = int(self.L.mi_rollout_batch_workspace_bytes(vae.dev.handle, ppo.dev.handle, E))
        if self.scratch_bytes <= 0:
            raise milib.MiError("mi_rollout_batch_workspace_bytes: " + self.L.cdll.mi_last_error().decode())
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=self.device)
        self._in_np = self.h_in.numpy()
        self._f_np = self._in_np[self._f_off:].view(np.float32)
        self._out_np = self.h_out.numpy().reshape(E, self.row)
        self._rng = np.random.Generator(np.random.Philox(int(seed if seed is not None else (ppo.seed or 0)) + 0xAC7))

    def __call__(self, frames_u8, measurements, greedy=False, noise=None):
        f = np.asarray(frames_u8)
        if f.dtype != np.uint8 or f.ndim < 1 or f.size != f.shape[0] * self.frame_bytes:
            raise ValueError("BatchedRolloutStep: expected uint8 frames [n, ...] of %d bytes each" % self.frame_bytes)
        n = int(f.shape[0])
        if not 1 <= n <= self.num_envs:
            raise ValueError("BatchedRolloutStep: 1 <= n <= num_envs = %d, got %d" % (self.num_envs, n))
        meas = np.asarray(measurements, np.float64)
        if meas.shape != (n, self.n_meas):
            raise ValueError("BatchedRolloutStep: expected measurements [%d, %d]" % (n, self.n_meas))
        nm, na = n * self.n_meas, n * self.A
        if not greedy:
            nz = self._rng.standard_normal((n, self.A)) if noise is None else np.asarray(noise, np.float32)
            if nz.shape != (n, self.A):
                raise ValueError("BatchedRolloutStep: expected noise [%d, %d]" % (n, self.A))
            self._f_np[nm:nm + na] = nz.reshape(-1)
        self._in_np[:n * self.frame_bytes] = f.reshape(-1)
        self._f_np[:nm] = meas.reshape(-1)                                           # f64 -> f32 at the feed, as ppo.py:108-109
        import torch
        st = torch.cuda.current_stream(self.device)
        used = self._f_off + 4 * (nm + na)
        if self.d_in is not None:
            self.d_in[:used].copy_(self.h_in[:used], non_blocking=True)
        base = (self.h_in if self.d_in is None else self.d_in).data_ptr()
        fptr = base + self._f_off
        self.L.mi_rollout_step_batch(self.vae.dev.handle, self.ppo.dev.handle, st.cuda_stream, base, fptr, self.n_meas, None if greedy else fptr + 4 * nm,
                                     1 if greedy else 0, n, self.scratch.data_ptr(), self.scratch_bytes, (self.h_out if self.d_out is None else self.d_out).data_ptr())
        if self.d_out is not None:
            self.h_out[:n * self.row].copy_(self.d_out[:n * self.row], non_blocking=True)
        st.synchronize()
        o = self._out_np[:n]
        actions, values = o[:, :self.A].copy(), o[:, self.A].copy()
        states = np.concatenate([o[:, self.A + 1:].astype(np.float64), meas], axis=1)
        return actions, values, states
