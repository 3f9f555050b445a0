"""CPU-only tests of global-norm gradient clipping (mi_ppo_set_max_grad_norm / mi_ppo_max_grad_norm / mi_ppo_grad_norm, PPO.set_max_grad_norm, the rollout buffers'
grad_norms): the C-ABI surface and every argument error the host can reach without an engine, PPO.set_max_grad_norm's validation on an object without a session and
the MI355_PPO_MAX_GRAD_NORM knob, the pinned signatures, and the gfx950 code of elementwise.hip (compiled here, no GPU needed): the three new kernels exist under
names of their own beside adam_tf_kernel and use no private segment."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

from rollout_host_common import ROOT, _kernel, _listing
from test_rollout_diagnostics_host import OLD_FUSED


def test_entry_points_are_declared_and_exported():
    from mi355 import lib as milib
    protos = milib.parse_header()
    assert protos["mi_ppo_set_max_grad_norm"] == ("int", [("void*", "h"), ("float", "max_norm")])
    assert protos["mi_ppo_max_grad_norm"] == ("float", [("void*", "h")])
    assert protos["mi_ppo_grad_norm"] == ("int", [("void*", "h"), ("void*", "stream"), ("float", "max_norm")])
    L = milib.get()
    for name in ("mi_ppo_set_max_grad_norm", "mi_ppo_max_grad_norm", "mi_ppo_grad_norm"):
        assert hasattr(L.cdll, name), name
    assert L.mi_abi_version() == 7
    text = open(milib.HEADER).read()
    i = text.index("int mi_ppo_set_max_grad_norm")
    comment = text[text.rfind("/*", 0, i):i]
    for c in ("clip_by_global_norm", "sqrt(sumsq)", "(double)g * (double)g", "alignment", "rounded to fp32", "no atomics", "bitwise equal", "NOT modified", "NOT written",
              "optimiser state", "+inf", "non-finite", "mi_ppo_buffer(h, 2)", "mi_ppo_train_step_dp", "all-reduce", "256 rows", "exactly the launches"):
        assert c in comment, c


def test_every_host_checkable_argument_error():
    """A null handle is a state error; the limit is checked before the engine is looked at, so a dummy handle is never dereferenced.  Each message starts with the
    entry's name."""
    from mi355 import lib as milib
    L = milib.get()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    err = L.cdll.mi_last_error
    f = ctypes.c_float
    assert L.cdll.mi_ppo_set_max_grad_norm(None, f(0.5)) == -4 and err() == b"mi_ppo_set_max_grad_norm: null handle"
    assert L.cdll.mi_ppo_set_max_grad_norm(None, f(-1.0)) == -4                        # the handle first
    for bad in (-1.0, -0.5, float("-inf"), float("nan")):
        assert L.cdll.mi_ppo_set_max_grad_norm(p, f(bad)) == -1 and err().startswith(b"mi_ppo_set_max_grad_norm: max_norm"), bad
    assert L.cdll.mi_ppo_grad_norm(None, None, f(0.5)) == -4 and err() == b"mi_ppo_grad_norm: null handle"
    assert L.cdll.mi_ppo_grad_norm(None, None, f(float("nan"))) == -4
    for bad in (-1.0, float("-inf"), float("nan"), 0.0):
        assert L.cdll.mi_ppo_grad_norm(p, None, f(bad)) == -1 and err().startswith(b"mi_ppo_grad_norm: max_norm"), bad
    assert L.cdll.mi_ppo_max_grad_norm(None) == -1.0 and err() == b"mi_ppo_max_grad_norm: null handle"
    assert all(x == 0.0 for x in buf)                                                  # the dummy handle was not written either
    # the checked binding raises with the entry's name
    with pytest.raises(milib.MiError, match="mi_ppo_set_max_grad_norm failed"):
        L.mi_ppo_set_max_grad_norm(None, 1.0)
    # the neighbour keeps its message
    assert L.cdll.mi_ppo_apply_adam(None, None, f(1e-4), f(0.9), f(0.999), f(1e-8)) == -4 and err() == b"ppo engine: null handle"


class _Space:
    shape = (2,)
    low = np.array([-1.0, 0.0], np.float32)
    high = np.array([1.0, 1.0], np.float32)


def make_ppo(tmp_path):
    from ppo import PPO
    return PPO(np.array([67]), _Space(), model_dir=str(tmp_path))


def test_set_max_grad_norm_validation_without_a_session(tmp_path, monkeypatch):
    monkeypatch.delenv("MI355_PPO_MAX_GRAD_NORM", raising=False)
    m = make_ppo(tmp_path)
    assert m.max_grad_norm is None and m.dev is None
    for good, want in ((0.5, 0.5), (3, 3.0), (np.float32(0.25), 0.25), (float("inf"), float("inf")), (None, None)):
        m.set_max_grad_norm(good)
        assert m.max_grad_norm == want and (want is None or isinstance(m.max_grad_norm, float))
    m.set_max_grad_norm(0.5)
    for bad in (0, 0.0, -0.5, float("nan"), -float("inf"), True, False, "0.5", [0.5]):
        with pytest.raises(ValueError, match=r"PPO\.set_max_grad_norm: the value is None or a positive float"):
            m.set_max_grad_norm(bad)
        assert m.max_grad_norm == 0.5 and m.dev is None, bad                           # refused before anything changed or touched a device
    with pytest.raises(RuntimeError, match="init_session"):
        m.last_grad_norm()
    # not part of a checkpoint's keys: state_dict needs a session, so look at the source of truth instead
    assert "max_grad_norm" not in inspect.getsource(type(m).state_dict) and "max_grad_norm" not in inspect.getsource(type(m).load_state_dict)


def test_the_environment_knob(tmp_path, monkeypatch):
    for text, want in (("0.5", 0.5), (" 2 ", 2.0), ("inf", float("inf")), ("1e-3", 1e-3), ("", None), ("   ", None)):
        monkeypatch.setenv("MI355_PPO_MAX_GRAD_NORM", text)
        assert make_ppo(tmp_path).max_grad_norm == want, text
    monkeypatch.delenv("MI355_PPO_MAX_GRAD_NORM")
    assert make_ppo(tmp_path).max_grad_norm is None
    for text in ("0", "-1", "nan", "half", "-inf"):
        monkeypatch.setenv("MI355_PPO_MAX_GRAD_NORM", text)
        with pytest.raises(ValueError, match="MI355_PPO_MAX_GRAD_NORM"):
            make_ppo(tmp_path)
    # set_max_grad_norm overrides what the knob supplied
    monkeypatch.setenv("MI355_PPO_MAX_GRAD_NORM", "0.5")
    m = make_ppo(tmp_path)
    m.set_max_grad_norm(None)
    assert m.max_grad_norm is None
    assert "MI355_PPO_MAX_GRAD_NORM" in open(os.path.join(ROOT, "DESIGN.md")).read()              # the Python-side knob table


def test_the_one_validation_function():
    from mi355.lib import max_grad_norm_value
    assert max_grad_norm_value(None) is None and max_grad_norm_value(2) == 2.0 and math.isinf(max_grad_norm_value(float("inf")))
    for bad in (0, -1.0, float("nan"), True, "1", [1.0]):
        with pytest.raises(ValueError, match="who: the value is None or a positive float"):
            max_grad_norm_value(bad, "who")


def test_pinned_signatures_are_unchanged():
    import rollout
    from mi355.ppo_device import PpoDevice
    from ppo import PPO
    from rollout import ContinuousRolloutBuffer as C, RolloutBuffer as B
    sig = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert sig(PPO.__init__) == ["self", "input_shape", "action_space", "learning_rate", "lr_decay", "epsilon", "value_scale", "entropy_scale", "initial_std", "model_dir",
                                 "seed", "precision"]
    assert sig(B.update) == ["self", "gamma", "lam", "num_epochs", "batch_size", "stage_times"]
    assert sig(B.update_with_diagnostics) == sig(B.update) + ["target_kl"]
    assert sig(C.update) == ["self", "gamma", "lam", "num_epochs", "batch_size", "normalize", "stage_times"]
    assert sig(C.update_with_diagnostics) == sig(C.update) + ["target_kl"]
    assert sig(B.step) == ["self", "frames_u8", "measurements", "env_ids", "greedy", "noise"] == sig(C.step)
    assert sig(PPO.set_max_grad_norm) == ["self", "value"] and sig(PPO.last_grad_norm) == ["self"]
    assert sig(PpoDevice.set_max_grad_norm) == ["self", "max_norm"] and sig(PpoDevice.grad_norm) == ["self", "max_norm"]
    assert sig(PpoDevice.apply_adam) == ["self", "alpha", "beta1", "beta2", "epsilon"]
    for c in ("set_max_grad_norm(0.5)", "MI355_PPO_MAX_GRAD_NORM", "grad_norms", "clip_scales", "grad_norm_max", "clipped_steps", "no atomics"):
        assert c in rollout.__doc__, c


ANON = r"_ZN12_GLOBAL__N_1"
NEW_KERNELS = [ANON + r"17grad_sumsq_kernelE", ANON + r"23grad_norm_finish_kernelE", ANON + r"22adam_tf_clipped_kernelE"]


def test_the_new_kernels_in_the_gfx950_listing():
    text = _listing("elementwise")
    for prefix, static_lds in zip(NEW_KERNELS, (4 * 8, 0, 0)):
        name, body, scratch, lds = _kernel(text, prefix)
        assert scratch == 0, name                                                    # no private segment: nothing spills, the table stays in the kernel arguments
        assert lds == static_lds, name                                               # one double per wave in the sum's block reduction, nothing else
        assert "atomic" not in body, name                                            # ordered sums only
    name, body, _, _ = _kernel(text, NEW_KERNELS[0])
    assert "global_load_dwordx4" in body and ("v_fma_f64" in body or "v_mul_f64" in body), name    # 16-byte loads, fp64 accumulation
    name, body, _, _ = _kernel(text, NEW_KERNELS[2])
    assert "v_mul_f32" in body, name                                                 # g * scale is a multiply of its own in front of the update
    _kernel(text, ANON + r"14adam_tf_kernelE")                                       # the VAE path's optimiser keeps its name
    fused = _listing("ppo_fused")
    for prefix in OLD_FUSED:
        _kernel(fused, prefix)
