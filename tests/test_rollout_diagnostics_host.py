"""CPU-only tests of the update diagnostics (mi_ppo_update_stats_idx / mi355.ppo_device.update_stats_summary / rollout.RolloutBuffer.update_with_diagnostics): the
C-ABI surface and every argument error the host can check without an engine, the scratch size, the sums-to-dict function against numpy, the ValueErrors of
update_with_diagnostics that need no device, update() left as it was, and the gfx950 code of ppo_fused.hip (compiled here, no GPU needed): the two new kernels
exist under names of their own beside the old ones and spill nothing."""
import ctypes
import inspect
import math
import re

import numpy as np
import pytest

from rollout_host_common import _kernel, _listing


STATS_ARGS = [("void*", "h"), ("void*", "stream"), ("const float*", "states"), ("const float*", "actions"), ("const float*", "returns"), ("const float*", "logp_old"),
              ("const int*", "row_idx"), ("int", "n_rows"), ("int", "M"), ("int", "accumulate"), ("double*", "scratch"), ("double*", "stats"),
              ("float*", "logp_new_out"), ("float*", "value_out")]


def n_stats():
    from mi355 import lib as milib
    return int(re.search(r"#define\s+MI_PPO_N_STATS\s+(\d+)", open(milib.HEADER).read()).group(1))


def test_entry_points_are_declared_and_exported():
    from mi355 import lib as milib
    from mi355 import ppo_device
    protos = milib.parse_header()
    assert protos["mi_ppo_update_stats_scratch_doubles"] == ("long long", [("int", "M")])
    assert protos["mi_ppo_update_stats_idx"] == ("int", STATS_ARGS)
    L = milib.get()
    assert hasattr(L.cdll, "mi_ppo_update_stats_idx") and hasattr(L.cdll, "mi_ppo_update_stats_scratch_doubles")
    assert L.mi_abi_version() == 7
    assert n_stats() == 9 == ppo_device.N_STATS
    text = open(milib.HEADER).read()
    i = text.index("int mi_ppo_update_stats_idx")
    comment = text[text.rfind("/*", 0, i):i]
    for c in ("k3", "r - 1 - log r", "r - 1 - d", "|r - 1| > clip_eps", "(ret - v)^2", "ret^2", "explained variance", "logp_old", "accumulate", "NOT modified",
              "optimiser state", "gradient buffer", "losses", "action_mean", "no atomics", "bitwise equal", "row_idx"):
        assert c in comment, c


def test_every_host_checkable_argument_error():
    """A null handle is a state error; everything checked before the engine is looked at is MI_ERR_ARG with a message that starts with the entry's name.  The handle
    and the pointers here are never dereferenced: every call fails before the first check that needs the engine (M against max_batch; tested on the GPU)."""
    from mi355 import lib as milib
    L = milib.get()
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)
    fn, err = L.cdll.mi_ppo_update_stats_idx, L.cdll.mi_last_error
    names = [a[1] for a in STATS_ARGS]
    good = dict(h=p, stream=None, states=p, actions=p, returns=p, logp_old=p, row_idx=p, n_rows=8, M=4, accumulate=0, scratch=p, stats=p, logp_new_out=None,
                value_out=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return fn(*[a[n] for n in names])
    assert call(h=None) == -4 and err() == b"mi_ppo_update_stats_idx: null handle"
    assert call(h=None, states=None, M=0) == -4                                      # the handle first
    for missing in ("states", "actions", "returns", "logp_old", "row_idx", "scratch", "stats"):
        assert call(**{missing: None}) == -1 and err() == b"mi_ppo_update_stats_idx: missing buffers (" + missing.encode() + b")", missing
    for kw in (dict(M=0), dict(M=-3), dict(n_rows=0), dict(n_rows=-1)):
        assert call(**kw) == -1 and err().startswith(b"mi_ppo_update_stats_idx: batch outside [1, max_batch] or empty tables"), kw
    for bad in (2, -1, 7):
        assert call(accumulate=bad) == -1 and err().startswith(b"mi_ppo_update_stats_idx: accumulate"), bad
    # the neighbours keep their messages
    assert L.cdll.mi_ppo_train_step_idx(None, None, p, p, p, p, p, p, 8, 4, 1.0, 1.0, 1e-4, 0.9, 0.999, 1e-8) == -4 and err() == b"ppo engine: null handle"


def test_scratch_size():
    from mi355 import lib as milib
    L = milib.get()
    n = n_stats()
    last = 0
    for M in list(range(1, 200)) + [255, 256, 257, 1024, 4095, 4096, 4097, 1 << 20]:
        got = L.mi_ppo_update_stats_scratch_doubles(M)
        assert got > 0 and got >= last and got >= n * math.ceil(M / 32), M
        last = got
    for M in (0, -5):
        assert L.mi_ppo_update_stats_scratch_doubles(M) > 0, M


def sums_of(lp, lpo, ret, v, eps):
    d = lp - lpo
    r = np.exp(d)
    e = ret - v
    return np.array([len(d), d.sum(), (r - 1 - d).sum(), (np.abs(r - 1) > eps).sum(), r.sum(), ret.sum(), (ret * ret).sum(), e.sum(), (e * e).sum()], np.float64)


def test_sums_to_dict_against_numpy():
    from mi355.ppo_device import update_stats_summary
    rng = np.random.RandomState(3)
    n, eps = 37, 0.2
    lpo = rng.standard_normal(n)
    lp = lpo + 0.3 * rng.standard_normal(n)
    ret = 2.0 + rng.standard_normal(n)
    v = ret + 0.5 * rng.standard_normal(n)
    got = update_stats_summary(sums_of(lp, lpo, ret, v, eps))
    assert sorted(got) == sorted(["samples", "approx_kl", "approx_kl_k1", "clip_fraction", "ratio_mean", "value_mse", "explained_variance"])
    d, r = lp - lpo, np.exp(lp - lpo)
    assert got["samples"] == n and isinstance(got["samples"], int)
    assert got["approx_kl"] == pytest.approx(np.mean(r - 1 - np.log(r)), rel=1e-12)
    assert got["approx_kl_k1"] == pytest.approx(-np.mean(d), rel=1e-12)
    assert got["clip_fraction"] == np.mean(np.abs(r - 1) > eps) and 0 < got["clip_fraction"] < 1
    assert got["ratio_mean"] == pytest.approx(np.mean(r), rel=1e-12)
    assert got["value_mse"] == pytest.approx(np.mean((ret - v) ** 2), rel=1e-12)
    assert got["explained_variance"] == pytest.approx(1 - np.var(ret - v) / np.var(ret), rel=1e-10)
    # a perfect value net explains everything; one that is off by a constant still does (the variance of the error is 0)
    assert update_stats_summary(sums_of(lp, lpo, ret, ret, eps))["explained_variance"] == 1.0
    assert update_stats_summary(sums_of(lp, lpo, ret, ret - 0.5, eps))["explained_variance"] == pytest.approx(1.0, abs=1e-12)
    # Var(ret) = 0: no variance to explain
    const = update_stats_summary(sums_of(lp, lpo, np.full(n, 2.0), v, eps))
    assert math.isnan(const["explained_variance"]) and const["value_mse"] == pytest.approx(np.mean((2.0 - v) ** 2), rel=1e-12)
    # theta == theta_old
    same = update_stats_summary(sums_of(lpo, lpo, ret, v, eps))
    assert same["approx_kl"] == 0.0 and same["approx_kl_k1"] == 0.0 and same["clip_fraction"] == 0.0 and same["ratio_mean"] == 1.0
    # a float32 or list input is taken as it is; a wrong length or an empty count is refused
    assert update_stats_summary(list(sums_of(lp, lpo, ret, v, eps)))["samples"] == n
    with pytest.raises(ValueError, match="expected 9 sums"):
        update_stats_summary(np.zeros(8))
    with pytest.raises(ValueError, match="no sample"):
        update_stats_summary(np.zeros(9))


class _Dev:
    def __init__(self, fused):
        self.fused = fused

    def fused_ok(self):
        return self.fused


class _Ppo:
    def __init__(self, fused):
        self.dev = _Dev(fused)

    def _need_dev(self):
        return self.dev


def stub(cls, fused=True):
    """A buffer object without a device behind it: what update_with_diagnostics looks at up to rows.check_update(), with the class's own (empty) book-keeping."""
    b = object.__new__(cls)
    b.ppo, b.rows, b.checked = _Ppo(fused), cls._rows_class(2, 4), []
    inner = b.rows.check_update

    def check_update():
        b.checked.append(1)
        inner()
    b.rows.check_update = check_update
    return b


def test_the_value_errors_of_update_with_diagnostics_that_need_no_device():
    from rollout import ContinuousRolloutBuffer, RolloutBuffer
    for cls in (RolloutBuffer, ContinuousRolloutBuffer):
        for bad in (0, 0.0, -0.01, float("nan"), float("inf"), -float("inf"), "0.02", True, [0.02]):
            b = stub(cls)
            with pytest.raises(ValueError, match=cls.__name__ + r"\.update_with_diagnostics: target_kl is None or a positive finite float"):
                b.update_with_diagnostics(target_kl=bad)
            assert not b.checked, bad
        # no cached log pi_old (the fused kernels do not take the policy's shape): refused before check_update() is reached
        for kl in (None, 0.02):
            b = stub(cls, fused=False)
            with pytest.raises(ValueError, match="cached log pi_old"):
                b.update_with_diagnostics(target_kl=kl)
            assert not b.checked
        # good arguments get as far as the book-keeping's own check
        for kl in (None, 0.02, np.float32(0.5), 3):
            b = stub(cls)
            with pytest.raises(ValueError, match="update with no samples"):
                b.update_with_diagnostics(target_kl=kl)
            assert len(b.checked) == 1
        # update() itself never asks for the fused kernels
        b = stub(cls, fused=False)
        with pytest.raises(ValueError, match="update with no samples"):
            b.update()
    with pytest.raises(ValueError, match="normalize is 'segment' or 'batch'"):
        stub(ContinuousRolloutBuffer).update_with_diagnostics(normalize="lane", target_kl=0.02)


def test_signatures_and_documents():
    import rollout
    from mi355.ppo_device import PpoDevice
    from rollout import ContinuousRolloutBuffer as C, RolloutBuffer as B
    sig = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    defaults = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if k != "self"}      # noqa: E731
    # update() keeps its arguments; the diagnostics form takes the same ones and target_kl
    assert sig(B.update_with_diagnostics) == sig(B.update) + ["target_kl"]
    assert sig(C.update_with_diagnostics) == sig(C.update) + ["target_kl"]
    for cls in (B, C):
        assert defaults(cls.update_with_diagnostics) == dict(defaults(cls.update), target_kl=None)
        doc = cls.update_with_diagnostics.__doc__ + B.update_with_diagnostics.__doc__
        for c in ("plain `>`", "1.5 x", "np.random.shuffle", "once per epoch that RAN", "epochs_run", "stopped_early", "4096"):
            assert c in doc, c
    assert sig(PpoDevice.update_stats) == ["self", "states", "actions", "returns", "logp_old", "row_idx", "M", "stats", "scratch", "accumulate", "logp_new_out", "value_out"]
    d = defaults(PpoDevice.update_stats)
    assert d["accumulate"] is False and d["logp_new_out"] is None and d["value_out"] is None
    assert "update_with_diagnostics(num_epochs=10, batch_size=32, target_kl=0.03)" in rollout.__doc__ and "mi_ppo_update_stats_idx" in rollout.__doc__


NEW_HEAD = [r"_ZN2mi28ppo_update_stats_head_kernelILi2EE", r"_ZN2mi28ppo_update_stats_head_kernelILi8EE"]
NEW_REDUCE = r"_ZN2mi23ppo_stats_reduce_kernelILi9EE"                            # (one template behind both statistics kernels, here at MI_PPO_N_STATS: csrc/ppo_head.hpp)
OLD_FUSED = [r"_ZN2mi23ppo_predict_head_kernelILi2ELi3EE", r"_ZN2mi23ppo_predict_head_kernelILi8ELi3EE", r"_ZN2mi23ppo_predict_head_kernelILi2ELi6EE",
             r"_ZN2mi20ppo_head_loss_kernelILi2EE", r"_ZN2mi20ppo_head_loss_kernelILi8EE", r"_ZN2mi13ppo_l1_kernelILb0EE", r"_ZN2mi13ppo_l1_kernelILb1EE",
             r"_ZN2mi13ppo_l2_kernelILb0EE", r"_ZN2mi13ppo_l2_kernelILb1EE", r"_ZN2mi14ppo_dh1_kernelILb0EE", r"_ZN2mi16ppo_wgrad_kernelILb1ELb0EE"]


def test_the_new_kernels_in_the_gfx950_listing():
    text = _listing("ppo_fused")
    for prefix in NEW_HEAD:
        name, body, scratch, static_lds = _kernel(text, prefix)
        assert scratch == 0, name                                                    # no private segment: nothing spills
        assert static_lds == 4 * n_stats() * 8, name                                 # one row of partial sums per wave, nothing else
    name, body, scratch, static_lds = _kernel(text, NEW_REDUCE)
    assert scratch == 0 and static_lds == 0, name
    for prefix in OLD_FUSED:                                                         # the old kernels keep their names
        _kernel(text, prefix)
