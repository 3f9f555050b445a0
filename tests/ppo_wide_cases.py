"""PPO problems at more than 96 inputs -- the widths mi_ppo_set_wide_inputs opens to the fused kernels -- with their float64 reference (test infrastructure; used by
test_ppo_wide_host.py and test_zzzzz_ppo_wide_inputs_gpu.py).  The builders, the reference and the tolerances are those of tests/ppo_shape_cases.py, imported.

  name    inputs -> hidden, actions   kin    why
  W100    100 -> (64, 64), 3          104    first width past the old range; 13 k-steps deal 4 / 4 / 4 / 1
  W131    131 -> (36, 20), 2          136    z_dim 128; din % 8 = 3; split mode: 9 k-blocks, wave 3 has none; H1 a partial tile
  W259    259 -> (132, 320), 3        264    33 steps, uneven shares; H1 / H2 at the tile and LDS limits
  W515    515 -> (500, 300), 2        520    z_dim 512 on the reference trunk; a share of 17 steps is a second chunk of the K-split kernel
  W1024   1024 -> (64, 64), 8         1024   the upper limit
  W1025   1025 -> (64, 64), 2         1032   past the limit: the per-layer path in every mode

M = 5 / 33 / 77 each (W1025: 33), and 257 at W131 and W515 (engines of max_batch 320: the gradient slabs of minibatches above 256 rows).

The weight scale of a case is its perturbation theta - theta_old: log r sums the change of din x H1 first-layer weights, so the perturbation shrinks with
sqrt(67 / din) and 1 / sqrt(actions) from the 0.03 of the reference shape.  (seed, perturb) are pinned below, found once by a search over seeds and a few multiples of
that scale; the first hit was taken, nothing searches at test time.  What the float64 reference of every case satisfies (test_ppo_wide_host.py asserts it):
  - ppo_shape_cases.conditions_met: 10 % .. 60 % of the samples on the zero-slope branch of min(r A, clip(r) A), at least one on each side -- so the clipped
    fraction lies strictly between 0 and 1 --, no ratio within 1e-3 of a clip edge, every ratio inside [1 / 20, 20];
  - no action mean saturates: every mean keeps at least 1 % of its action's range from both bounds (SATURATION_MARGIN).
"""
from collections import OrderedDict

import numpy as np

import ppo_shape_cases as pc

KIN_NARROW, KIN_WIDE, H2_MAX, ACT_MAX = 96, 1024, 320, 8
SATURATION_MARGIN = 0.01

# name -> (input_dim, num_actions, hidden)
SHAPES = OrderedDict([
    ("W100", (100, 3, (64, 64))), ("W131", (131, 2, (36, 20))), ("W259", (259, 3, (132, 320))), ("W515", (515, 2, (500, 300))),
    ("W1024", (1024, 8, (64, 64))), ("W1025", (1025, 2, (64, 64))),
])
# name-M -> (seed, perturb)
PINNED = OrderedDict([
    ("W100-5", (10, 0.02835)), ("W100-33", (5, 0.01418)), ("W100-77", (1, 0.02835)),
    ("W131-5", (22, 0.03034)), ("W131-33", (5, 0.03034)), ("W131-77", (11, 0.03034)), ("W131-257", (1, 0.04551)),
    ("W259-5", (36, 0.01233)), ("W259-33", (9, 0.00881)), ("W259-77", (4, 0.00881)),
    ("W515-5", (23, 0.0153)), ("W515-33", (18, 0.00765)), ("W515-77", (2, 0.0153)), ("W515-257", (6, 0.0153)),
    ("W1024-5", (21, 0.00543)), ("W1024-33", (3, 0.00543)), ("W1024-77", (3, 0.00543)),
    ("W1025-33", (10, 0.01627)),
])
WIDE_CASES = OrderedDict((k, SHAPES[k.split("-")[0]] + (int(k.split("-")[1]),) + v) for k, v in PINNED.items())
FUSED_WIDE = [k for k in WIDE_CASES if not k.startswith("W1025")]         # fused in modes 1 and 2; nothing here is fused in mode 0
SMALL_FUSED_WIDE = [k for k in FUSED_WIDE if WIDE_CASES[k][3] <= 256]      # the in-kernel Adam needs the whole minibatch in one wave
SLAB_CASES = [k for k in FUSED_WIDE if WIDE_CASES[k][3] > 256]


def kin_of(input_dim):
    return (input_dim + 7) // 8 * 8


def fused_in_mode(input_dim, num_actions, hidden, mode):
    """The range predicates of csrc/ppo_fused.hip restated: mode 0 -> mi_ppo_fused_shape_in_range, 1 / 2 -> mi_ppo_fused_shape_in_wide_range."""
    h2 = hidden[1]
    return 1 <= num_actions <= ACT_MAX and h2 <= H2_MAX and h2 % 4 == 0 and kin_of(input_dim) <= (KIN_WIDE if mode else KIN_NARROW)


def wave_shares(kin, split):
    """ppo_l1_wide_kernel's share arithmetic restated: the k-steps (of 8; split-bf16: k-blocks of 16) of kin dealt to the four waves as contiguous ranges
    -> [(begin, end)] x 4; an empty share has begin >= end."""
    steps = (kin + 15) // 16 if split else (kin + 7) // 8
    per = (steps + 3) // 4
    return [(w * per, min(steps, (w + 1) * per)) for w in range(4)]


def saturation_margin(c):
    """The smallest distance of a float64 action mean from its bounds, as a share of the action's range."""
    width = (c.high - c.low).astype(np.float64)
    return float((np.minimum(c.mean - c.low, c.high - c.mean) / width).min())


_BUILT = {}


def wide_case(name):
    """The problem of WIDE_CASES[name], built once per process and not to be modified."""
    if name not in _BUILT:
        _BUILT[name] = pc.build(*WIDE_CASES[name])
    return _BUILT[name]
