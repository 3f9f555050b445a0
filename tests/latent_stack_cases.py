"""Latent stacking (rollout.py: latent_stack=k; csrc/rollout.hip: rollout_stack_kernel) -- the shapes the tests run at, and a numpy restatement of what the kernel
does to a row and to a lane's history (test infrastructure; used by test_latent_stack_host.py and test_zzzzzz_latent_stack_gpu.py).  numpy only.

    row_e  = [ z_e | old_1 | .. | old_{k-1} | measurements_e ],   old_i = first_e ? z_e : hist[lane_e][i - 1]
    hist'[lane_e] = [ z_e | old_1 | .. | old_{k-2} ]              only with `advance`; a lane outside [0, n_lanes) is `first` and nothing of it is read or written

Everything is copying, so every statement below is bitwise: float32 in, float32 out, np.where for the select (NaN on the side that is not taken stays there)."""
import numpy as np

# (z_dim, k, n_meas): the smallest shapes that reach each edge of the kernel (128 threads, at most 8 columns per thread)
KERNEL_SHAPES = [
    (8, 15, 7),      # din 127: below the 128-thread stride
    (8, 16, 0),      # din 128: at the stride, no measurements
    (8, 16, 1),      # din 129: past the stride, a second trip
    (8, 2, 3),       # din 19: k = 2, where the shift has nothing to move
    (8, 3, 5),       # din 29
    (64, 4, 3),      # din 259: the shipped agent's stacked shape
    (64, 16, 0),     # din 1024: 8 values per thread, the maximum
]
BUFFER_SHAPES = [(3, 5), (5, 20)]                                                    # (E, T)
BUFFER_STACKS = [2, 4]


def din_of(z_dim, k, n_meas):
    return k * z_dim + n_meas


def stack_rows(hist, lanes, first, z, meas):
    """The rows of one call: hist float32 [n_lanes, k - 1, z_dim], lanes int [n], first bool-like [n], z float32 [n, z_dim], meas [n, n_meas]
    -> float32 [n, k z_dim + n_meas]."""
    hist, z = np.asarray(hist, np.float32), np.asarray(z, np.float32)
    n_lanes, km1, z_dim = hist.shape
    n = z.shape[0]
    meas = np.asarray(meas, np.float32).reshape(n, -1)
    rows = np.empty((n, (km1 + 1) * z_dim + meas.shape[1]), np.float32)
    for e in range(n):
        lane = int(lanes[e])
        inside = 0 <= lane < n_lanes
        fresh = bool(first[e]) or not inside
        old = hist[lane] if inside else np.zeros((km1, z_dim), np.float32)
        old = np.where(fresh, np.broadcast_to(z[e], (km1, z_dim)), old)
        rows[e] = np.concatenate([z[e], old.reshape(-1), meas[e]])
    return rows


def shift(hist, lanes, first, z, advance=True):
    """The history after that call (a new array): the lanes of the call take [z | their first k - 2 older latents]; with advance False, or for a lane outside the
    history, nothing changes."""
    hist = np.array(hist, np.float32)
    if not advance:
        return hist
    n_lanes, km1, z_dim = hist.shape
    rows = stack_rows(hist, lanes, first, z, np.zeros((len(lanes), 0), np.float32))
    for e, lane in enumerate(lanes):
        if 0 <= int(lane) < n_lanes:
            hist[int(lane)] = rows[e, :km1 * z_dim].reshape(km1, z_dim)
    return hist


class HostStack:
    """The host's picture of a step class with latent stacking on: the history and the fresh flags, driven by the latents the device RETURNED."""

    def __init__(self, num_envs, k, z_dim):
        self.k, self.z_dim = k, z_dim
        self.hist = np.zeros((num_envs, k - 1, z_dim), np.float32)
        self.fresh = np.ones(num_envs, bool)

    def call(self, lanes, z, meas, advance=True):
        """-> the rows the kernel must have assembled; advances like the step does."""
        lanes = np.asarray(lanes)
        rows = stack_rows(self.hist, lanes, self.fresh[lanes], z, meas)
        if advance:
            self.hist = shift(self.hist, lanes, self.fresh[lanes], z)
            self.fresh[lanes] = False
        return rows

    def restart(self, lanes=None):
        self.fresh[slice(None) if lanes is None else np.asarray(lanes)] = True
