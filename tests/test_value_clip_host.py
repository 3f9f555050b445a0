"""CPU-only tests of PPO2-style value-function clipping (mi_ppo_train_step_vclip, mi_ppo_value_clip_stats, PPO.set_value_clip, the rollout buffers' three
diagnostics keys): the C-ABI surface and every argument error the host can reach without an engine, PPO.set_value_clip's validation on an object without a session,
the new keyword of PPO._step_rows and the pinned signatures, value_clip_summary's arithmetic, and the gfx950 code of ppo_fused.hip / ppo_ops.hip (compiled here, no
GPU needed): the new kernels exist under names of their own, use no private segment, the clipped head kernels take the plain ones' LDS, and every older fused kernel
keeps its name."""
import ctypes
import inspect
import math

import numpy as np
import pytest

from rollout_host_common import _kernel, _listing
from test_rollout_diagnostics_host import OLD_FUSED

F = "const float*"
STEP_PROTO = ("int", [("void*", "h"), ("void*", "comm"), ("void*", "stream"), (F, "states"), (F, "actions"), (F, "returns"), (F, "advantage"), (F, "logp_old"),
                      (F, "old_values"), ("float", "clip_range_vf"), ("const int*", "row_idx"), ("int", "n_rows"), ("int", "M"), ("float", "inv_m"),
                      ("float", "grad_scale"), ("int", "adam"), ("float", "alpha"), ("float", "beta1"), ("float", "beta2"), ("float", "epsilon")])
STATS_PROTO = ("int", [("void*", "stream"), (F, "values_new"), (F, "old_values"), (F, "returns"), ("const int*", "row_idx"), ("int", "n_rows"), ("int", "M"),
                       ("float", "clip_range_vf"), ("int", "accumulate"), ("double*", "scratch"), ("double*", "stats")])


def test_entry_points_are_declared_and_exported():
    from mi355 import lib as milib
    from mi355 import ppo_device
    protos = milib.parse_header()
    assert protos["mi_ppo_train_step_vclip"] == STEP_PROTO
    assert protos["mi_ppo_value_clip_stats_scratch_doubles"] == ("long long", [("int", "M")])
    assert protos["mi_ppo_value_clip_stats"] == STATS_PROTO
    L = milib.get()
    for name in ("mi_ppo_train_step_vclip", "mi_ppo_value_clip_stats_scratch_doubles", "mi_ppo_value_clip_stats"):
        assert hasattr(L.cdll, name), name
    assert L.mi_abi_version() == 7
    text = open(milib.HEADER).read()
    assert "#define MI_PPO_N_VCLIP_STATS 4" in text and ppo_device.N_VCLIP_STATS == 4
    i = text.index("int mi_ppo_train_step_vclip")
    comment = text[text.rfind("/*", 0, i):i]
    for c in ("V_c  = min(max(V, V_old - eps_v), V_old + eps_v)", "bit for bit", "max(l_u, l_c)", "(l_c > l_u) ? 0 : 2 * value_scale * (V - R) / M_global", "tf.maximum",
              "first argument", "+inf", "losses[1]", "policy side", "row_idx == NULL", "mi_ppo_train_step_dp", "adam == 0", "mi_ppo_apply_adam", "no atomics",
              "no per-layer form", "mi_ppo_update_stats_idx", "not read"):
        assert c in comment, c
    # the scratch size needs no engine: one row of sums per block of 256 samples, at least one
    sd = L.mi_ppo_value_clip_stats_scratch_doubles
    assert [sd(m) for m in (-3, 0, 1, 256, 257, 4096)] == [4, 4, 4, 4, 8, 64]


def test_every_host_checkable_argument_error():
    """A null handle is a state error; what needs no engine is checked before the handle is looked at, so a dummy handle is never dereferenced.  Each message starts
    with the entry's name."""
    from mi355 import lib as milib
    L = milib.get()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    err = L.cdll.mi_last_error
    f = ctypes.c_float
    step = L.cdll.mi_ppo_train_step_vclip

    def call(h=p, old=p, eps=0.2, rows=None, n_rows=0, M=5, adam=1):
        return step(h, None, None, p, p, p, p, None, old, f(eps), rows, n_rows, M, f(0.2), f(1.0), adam, f(1e-4), f(0.9), f(0.999), f(1e-8))
    assert call(h=None) == -4 and err() == b"mi_ppo_train_step_vclip: null handle"
    assert call(h=None, M=0, old=None, eps=-1.0) == -4                                 # the handle first
    for M in (0, -1):
        assert call(M=M) == -1 and err().startswith(b"mi_ppo_train_step_vclip: batch outside [1, max_batch]"), M
    for n_rows in (0, -4):
        assert call(rows=p, n_rows=n_rows) == -1 and err().startswith(b"mi_ppo_train_step_vclip: batch outside [1, max_batch] or empty tables"), n_rows
    assert call(old=None) == -1 and err().startswith(b"mi_ppo_train_step_vclip: missing old_values")
    for bad in (0.0, -0.2, float("-inf"), float("nan")):
        assert call(eps=bad) == -1 and err().startswith(b"mi_ppo_train_step_vclip: clip_range_vf"), bad
    for bad in (-1, 2, 7):
        assert call(adam=bad) == -1 and err().startswith(b"mi_ppo_train_step_vclip: adam"), bad
    assert call(eps=float("inf"), adam=3) == -1 and err().startswith(b"mi_ppo_train_step_vclip: adam")      # +inf is a valid range: the next check answers
    # the statistics entry takes no engine at all
    stats = L.cdll.mi_ppo_value_clip_stats

    def scall(v=p, vo=p, r=p, rows=p, n_rows=8, M=5, eps=0.2, acc=0, scratch=p, out=p):
        return stats(None, v, vo, r, rows, n_rows, M, f(eps), acc, scratch, out)
    for kw in (dict(M=0), dict(M=-2), dict(n_rows=0)):
        assert scall(**kw) == -1 and err().startswith(b"mi_ppo_value_clip_stats: empty input"), kw
    for name in ("v", "vo", "r", "rows", "scratch", "out"):
        assert scall(**{name: None}) == -1 and err().startswith(b"mi_ppo_value_clip_stats: missing buffers"), name
    for bad in (0.0, -1.0, float("nan")):
        assert scall(eps=bad) == -1 and err().startswith(b"mi_ppo_value_clip_stats: clip_range_vf"), bad
    for bad in (-1, 2):
        assert scall(acc=bad) == -1 and err().startswith(b"mi_ppo_value_clip_stats: accumulate"), bad
    assert all(x == 0.0 for x in buf)                                                  # the dummy buffers were not written
    with pytest.raises(milib.MiError, match="mi_ppo_train_step_vclip failed"):        # the checked binding raises with the entry's name
        L.mi_ppo_train_step_vclip(None, None, None, None, None, None, None, None, None, 0.2, None, 0, 5, 0.2, 1.0, 1, 1e-4, 0.9, 0.999, 1e-8)
    # the neighbour keeps its message
    assert L.cdll.mi_ppo_train_step(None, None, p, p, p, p, None, 5, f(0.2), f(1.0), f(1e-4), f(0.9), f(0.999), f(1e-8)) == -4 and err() == b"ppo engine: null handle"


class _Space:
    shape = (2,)
    low = np.array([-1.0, 0.0], np.float32)
    high = np.array([1.0, 1.0], np.float32)


def make_ppo(tmp_path):
    from ppo import PPO
    return PPO(np.array([67]), _Space(), model_dir=str(tmp_path))


def test_set_value_clip_validation_without_a_session(tmp_path):
    m = make_ppo(tmp_path)
    assert m.value_clip is None and m.dev is None
    for good, want in ((0.2, 0.2), (3, 3.0), (np.float32(0.25), 0.25), (float("inf"), float("inf")), (None, None)):
        m.set_value_clip(good)
        assert m.value_clip == want and (want is None or isinstance(m.value_clip, float))
    m.set_value_clip(0.2)
    for bad in (0, 0.0, -0.5, float("nan"), -float("inf"), True, False, "0.2", [0.2]):
        with pytest.raises(ValueError, match=r"PPO\.set_value_clip: the value is None or a positive float"):
            m.set_value_clip(bad)
        assert m.value_clip == 0.2 and m.dev is None, bad                              # refused before anything changed or touched a device
    # train() / train_step() take no old values: they say so instead of running an unclipped step
    x = np.zeros((4, 67), np.float32), np.zeros((4, 2), np.float32), np.zeros(4, np.float32), np.zeros(4, np.float32)
    for fn in (m.train, m.train_step, m.learn):
        with pytest.raises(ValueError, match="value clipping is on"):
            fn(*x)
    m.set_value_clip(None)
    with pytest.raises(RuntimeError, match="init_session"):                            # off: the call is today's
        m.train(*x)
    # not part of a checkpoint, and no environment knob
    src = inspect.getsource(type(m))
    assert "value_clip" not in inspect.getsource(type(m).state_dict) and "value_clip" not in inspect.getsource(type(m).load_state_dict)
    assert "VALUE_CLIP" not in src and "CLIP_RANGE_VF" not in src


def test_the_one_validation_function():
    from mi355.lib import value_clip_value
    assert value_clip_value(None) is None and value_clip_value(2) == 2.0 and math.isinf(value_clip_value(float("inf")))
    for bad in (0, -1.0, float("nan"), True, "1", [1.0]):
        with pytest.raises(ValueError, match="who: the value is None or a positive float"):
            value_clip_value(bad, "who")


def test_signatures():
    import rollout
    from mi355.ppo_device import PpoDevice
    from ppo import PPO
    from rollout import ContinuousRolloutBuffer as C, RolloutBuffer as B
    sig = inspect.signature
    names = lambda f: list(sig(f).parameters)      # noqa: E731
    assert names(PPO._step_rows) == ["self", "s_all", "a_all", "r_all", "adv_all", "logp_old_all", "rows", "m_local", "m_global", "old_values_all"]
    assert sig(PPO._step_rows).parameters["old_values_all"].default is None
    assert names(PPO.set_value_clip) == ["self", "value"]
    assert names(PpoDevice.train_step_vclip) == ["self", "comm_handle", "states", "actions", "returns", "advantage", "logp_old", "old_values", "clip_range_vf", "row_idx",
                                                 "M", "inv_m", "grad_scale", "alpha", "beta1", "beta2", "epsilon", "adam"]
    assert names(PpoDevice.value_clip_stats) == ["self", "values_new", "old_values", "returns", "row_idx", "M", "clip_range_vf", "stats", "scratch", "accumulate"]
    # pinned by the older tests, unchanged here
    assert names(B.update) == ["self", "gamma", "lam", "num_epochs", "batch_size", "stage_times"]
    assert names(B.update_with_diagnostics) == names(B.update) + ["target_kl"]
    assert names(C.update) == ["self", "gamma", "lam", "num_epochs", "batch_size", "normalize", "stage_times"]
    assert names(C.update_with_diagnostics) == names(C.update) + ["target_kl"]
    assert names(PPO.train) == ["self", "input_states", "taken_actions", "returns", "advantage"] == names(PPO.train_step)
    assert names(PpoDevice.train_step_idx)[:7] == ["self", "states", "actions", "returns", "advantage", "logp_old", "row_idx"]
    for c in ("set_value_clip(0.2)", "value_clip_fraction", "value_loss_clipped", "value_grad_zero_fraction", "mi_ppo_train_step_vclip", "no environment knob"):
        assert c in rollout.__doc__, c


def test_step_rows_refuses_old_values_with_the_setting_off(tmp_path):
    m = make_ppo(tmp_path)
    m.dev = object()                                                                   # never looked at: the refusal comes first
    with pytest.raises(ValueError, match="value clipping is off"):
        m._step_rows(None, None, None, None, None, None, 4, 4, old_values_all=np.zeros(4, np.float32))


def test_value_clip_summary():
    from mi355.ppo_device import value_clip_summary
    out = value_clip_summary([8.0, 2.0, 6.0, 1.0])
    assert out == {"value_clip_fraction": 0.25, "value_loss_clipped": 0.75, "value_grad_zero_fraction": 0.125}
    for bad in ([1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], np.zeros(9)):
        with pytest.raises(ValueError, match="value_clip_summary"):
            value_clip_summary(bad)


MI = r"_ZN2mi"
PLAIN_HEAD = [MI + r"20ppo_head_loss_kernelILi2EE", MI + r"20ppo_head_loss_kernelILi8EE"]
CLIP_HEAD = [MI + r"26ppo_head_loss_vclip_kernelILi2EE", MI + r"26ppo_head_loss_vclip_kernelILi8EE"]
STATS_KERNELS = [MI + r"27ppo_value_clip_stats_kernelE", MI + r"28ppo_value_clip_reduce_kernelE"]


def test_the_new_kernels_in_the_gfx950_listing():
    fused = _listing("ppo_fused")
    for plain, clipped in zip(PLAIN_HEAD, CLIP_HEAD):
        p_name, p_body, p_scratch, p_lds = _kernel(fused, plain)
        c_name, c_body, c_scratch, c_lds = _kernel(fused, clipped)
        assert c_name != p_name and c_scratch == 0 and p_scratch == 0, (c_name, c_scratch)     # a kernel of its own, no private segment
        assert c_lds == p_lds and c_lds > 0, (c_name, c_lds, p_lds)                  # the plain kernel's LDS
        assert "atomic" not in c_body, c_name
        assert "v_max_f32" in c_body and "v_min_f32" in c_body, c_name               # the clamp of V and the larger of the two terms
    for prefix in OLD_FUSED:                                                         # the old kernels keep their names
        _kernel(fused, prefix)
    ops = _listing("ppo_ops")
    for prefix, static_lds in zip(STATS_KERNELS, (4 * 4 * 8, 0)):
        name, body, scratch, lds = _kernel(ops, prefix)
        assert scratch == 0, name
        assert lds == static_lds, name                                               # four doubles per wave in the block reduction, nothing else
        assert "atomic" not in body, name                                            # ordered sums only
    name, body, _, _ = _kernel(ops, STATS_KERNELS[0])
    assert "v_add_f64" in body and "v_mul_f64" in body, name                          # the terms are formed and summed in double
