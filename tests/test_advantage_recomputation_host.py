"""CPU-only tests of advantage recomputation (mi_ppo_values_idx / PpoDevice.values_idx / PPO.values / RolloutBuffer.set_advantage_recomputation): the setter and the
refusals that need no device, the C-ABI surface, the entry's refusals that need no engine, and the self-checks of tests/advantage_recomputation_cases.py -- its
float64 value net against the oracle's, its fp32 twin against the bound the GPU test asks of the device, and the three mutants of its update-with-refresh
reference against the bound they are checked under.  Also the gfx950 code of the new head kernel (compiled here, no GPU needed): no private segment, no LDS."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import advantage_recomputation_cases as ac
from oracle import ppo_oracle as po

VALUES_ARGS = [("void*", "h"), ("void*", "stream"), ("const float*", "states"), ("const int*", "row_idx"), ("long long", "n_rows"), ("long long", "M"),
               ("float*", "values_out")]


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
    """A buffer object without a device behind it: its class's own (empty) book-keeping and what the setter and _check_update look at."""
    b = object.__new__(cls)
    b.ppo, b.rows = _Ppo(fused), cls._rows_class(2, 4)
    b._adv_recompute = False
    b._reward_scaling = b._demo = None
    b.num_envs, b.horizon = 2, 4
    b.final_states = b._final_actions = b._final_raw_states = b.final_values_now = None
    return b


# ---------------------------------------------------------------------------------------------------------------------------------------- 1
def test_the_setter_takes_on_off_and_none():
    from rollout import RolloutBuffer
    b = stub(RolloutBuffer)
    assert list(inspect.signature(RolloutBuffer.set_advantage_recomputation).parameters) == ["self", "on"]
    assert inspect.signature(RolloutBuffer.set_advantage_recomputation).parameters["on"].default is True
    b.set_advantage_recomputation()
    assert b._adv_recompute is True
    for off in (False, None, np.bool_(False)):
        b.set_advantage_recomputation(True)
        b.set_advantage_recomputation(off)
        assert b._adv_recompute is False
    for bad in (1, 0, "on", 1.0, [True]):
        with pytest.raises(ValueError, match=r"RolloutBuffer\.set_advantage_recomputation: the value is True, False or None"):
            b.set_advantage_recomputation(bad)
        assert b._adv_recompute is False


@pytest.mark.parametrize("name", ["RolloutBuffer", "ContinuousRolloutBuffer"])
def test_the_setter_refuses_once_a_step_is_recorded(name):
    import rollout
    cls = getattr(rollout, name)
    b = stub(cls)
    b.rows.step_rows(None, 2)                                                        # a step awaits its outcome
    with pytest.raises(ValueError, match=name + r"\.set_advantage_recomputation: steps are recorded; call it after reset\(\)"):
        rollout.RolloutBuffer.set_advantage_recomputation(b, True)                   # (RolloutBuffer's: the subclass allocates its tables behind it)
    b.rows.outcome(np.zeros(2), np.zeros(2, bool))                                   # ... and counts
    for on in (True, False, None):
        with pytest.raises(ValueError, match="steps are recorded"):
            rollout.RolloutBuffer.set_advantage_recomputation(b, on)
    assert b._adv_recompute is False
    b.rows.reset()
    rollout.RolloutBuffer.set_advantage_recomputation(b, True)
    assert b._adv_recompute is True


def test_update_refuses_the_setting_without_the_fused_kernels():
    from rollout import ContinuousRolloutBuffer, RolloutBuffer
    for cls in (RolloutBuffer, ContinuousRolloutBuffer):
        b = stub(cls, fused=False)
        b._adv_recompute = True
        with pytest.raises(ValueError, match=cls.__name__ + r"\.update: advantage recomputation \(set_advantage_recomputation\) exists only in the fused kernels.*"
                                                            r"PPO\.set_wide_inputs\(\).*MI355_PPO_FUSED=0"):
            b._check_update(3, 4, None, None)
        b = stub(cls, fused=True)                                                    # with them: as far as the book-keeping's own check
        b._adv_recompute = True
        with pytest.raises(ValueError, match="update with no samples"):
            b._check_update(3, 4, None, None)
        b = stub(cls, fused=False)                                                   # with the setting off update() never asks for them
        with pytest.raises(ValueError, match="update with no samples"):
            b._check_update(3, 4, None, None)
    # update()'s signature is what it was
    assert list(inspect.signature(RolloutBuffer.update).parameters) == ["self", "gamma", "lam", "num_epochs", "batch_size", "stage_times"]
    assert list(inspect.signature(ContinuousRolloutBuffer.update).parameters) == ["self", "gamma", "lam", "num_epochs", "batch_size", "normalize", "stage_times"]


def test_documents():
    import rollout
    from mi355.ppo_device import PpoDevice
    from ppo import PPO
    assert list(inspect.signature(PpoDevice.values_idx).parameters) == ["self", "states", "row_idx", "M", "out"]
    assert list(inspect.signature(PPO.values).parameters) == ["self", "input_states"]
    for c in ("set_advantage_recomputation", "mi_ppo_values_idx", "values_now", "recomputed_epochs", "refreshed_values", "refreshed_final_values", "final_states"):
        assert c in rollout.__doc__, c
    assert "REFRESHED returns" in rollout.RolloutBuffer.update_with_diagnostics.__doc__


# ---------------------------------------------------------------------------------------------------------------------------------------- 2
def test_the_abi_has_the_new_entry_and_keeps_its_version():
    from mi355 import lib as milib
    protos = milib.parse_header()
    assert protos["mi_ppo_values_idx"] == ("int", VALUES_ARGS)
    L = milib.get()
    assert hasattr(L.cdll, "mi_ppo_values_idx")
    assert L.mi_abi_version() == 7
    text = open(milib.HEADER).read()
    i = text.index("int mi_ppo_values_idx")
    comment = text[text.rfind("/*", 0, i):i]
    for c in ("stores NOTHING", "max_batch", "bit for bit", "value_out", "mi_ppo_update_stats_idx", "NOT modified", "optimiser state", "gradient buffer", "losses",
              "no atomics", "row_idx == NULL", "MI_ERR_SHAPE", "2 GiB"):
        assert c in comment, c


# ---------------------------------------------------------------------------------------------------------------------------------------- 3
def test_the_refusals_that_need_no_engine():
    """On a NULL handle: what needs no engine is MI_ERR_ARG with its message -- the handle is looked at behind them, and only then is it a state error."""
    from mi355 import lib as milib
    L = milib.get()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    fn, err = L.cdll.mi_ppo_values_idx, L.cdll.mi_last_error
    names = [a[1] for a in VALUES_ARGS]
    good = dict(h=None, stream=None, states=p, row_idx=p, n_rows=8, M=4, values_out=p)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return fn(*[a[n] for n in names])
    MI_ERR_ARG, MI_ERR_STATE = -1, -4
    for kw in (dict(M=0), dict(M=-3), dict(n_rows=0), dict(n_rows=-1)):
        assert call(**kw) == MI_ERR_ARG and err().startswith(b"mi_ppo_values_idx: no rows (M < 1) or an empty table (n_rows < 1)"), kw
    assert call(states=None) == MI_ERR_ARG and err() == b"mi_ppo_values_idx: missing buffers (states)"
    assert call(values_out=None) == MI_ERR_ARG and err() == b"mi_ppo_values_idx: missing buffers (values_out)"
    assert call(row_idx=None, M=9) == MI_ERR_ARG and err().startswith(b"mi_ppo_values_idx: without a row list")
    assert call(row_idx=None, M=8) == MI_ERR_STATE and err() == b"mi_ppo_values_idx: null handle"      # M == n_rows is fine
    assert call(M=1 << 40) == MI_ERR_STATE                                           # a row list may be longer than the table, and than any max_batch
    assert call() == MI_ERR_STATE and err() == b"mi_ppo_values_idx: null handle"
    assert all(x == 0.0 for x in buf)


# ---------------------------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", list(ac.POLICIES))
def test_the_float64_value_net_is_the_oracles(name):
    pol = ac.policy(name)
    s = ac.states(name, 33)
    th = {k: torch.from_numpy(v.astype(np.float64)) for k, v in pol["theta"].items()}
    with torch.no_grad():
        _, _, v = po.policy_forward(th, torch.from_numpy(s.astype(np.float64)), pol["low"], pol["high"])
    err = np.abs(ac.value64(pol["theta"], s) - v.numpy()).max()
    print("%s: max |value64 - oracle| = %.3e" % (name, err))
    assert err <= 1e-12


@pytest.mark.parametrize("name", list(ac.POLICIES))
def test_the_fp32_twin_is_inside_the_bound_at_every_case(name):
    pol = ac.policy(name)
    for M in ac.ROW_COUNTS:
        s = ac.states(name, M)
        d = ac.distance(ac.value32(pol["theta"], s), ac.value64(pol["theta"], s))
        print("%s M=%d: fp32 twin at %.3e of the bound" % (name, M, d))
        assert d <= 1.0, (name, M, d)
    assert np.abs(ac.value64(pol["theta"], ac.states(name, 257))).max() > 0.01          # the values are not all next to zero: the relative part is asked too


def test_distance_sees_nan_in_other_places():
    assert ac.distance([1.0, np.nan], [1.0, np.nan]) == 0.0
    assert ac.distance([1.0, 2.0], [1.0, np.nan]) == float("inf") and ac.distance([1.0], [1.0, 2.0]) == float("inf")
    assert ac.distance([1.0 + 2.2e-4], [1.0]) == pytest.approx(2.0, rel=1e-3)


_REF = {}


def reference(mutant=None):
    if mutant not in _REF:
        _REF[mutant] = ac.update_reference(ac.refresh_case(), mutant=mutant)
    return _REF[mutant]


def test_the_reference_refreshes_before_every_epoch_but_the_first():
    case, ref = ac.refresh_case(), reference()
    assert ref["recomputed_epochs"] == 2
    raw, ret, adv = ac.finish64(case, case["values"], 0.99, 0.95)
    assert np.array_equal(ref["returns"], ret, equal_nan=True) and np.array_equal(ref["advantages"], adv, equal_nan=True)      # the first finish reads the recorded values
    rec = np.arange(case["T"])[None, :] < case["lengths"][:, None]
    assert np.array_equal(np.isnan(ref["refreshed_values"]), ~rec) and np.array_equal(np.isnan(ref["refreshed_returns"]), ~rec)
    assert ac.distance(ref["refreshed_returns"], ref["returns"]) > 10                # ... and the refresh moves them
    assert ac.update_reference(case, num_epochs=1)["recomputed_epochs"] == 0
    two = ac.update_reference(case)
    assert all(np.array_equal(two["params"][k], ref["params"][k]) for k in ref["params"])      # two runs


@pytest.mark.parametrize("mutant", ac.MUTANTS)
def test_every_mutant_is_seen_at_ten_times_the_bound(mutant):
    d = ac.mutant_distance(reference(), reference(mutant))
    print("%s: %.3e x the bound" % (mutant, d))
    assert d >= 10.0, (mutant, d)


# ---------------------------------------------------------------------------------------------------------------------------------------- the kernel
def test_the_value_head_kernel_in_the_gfx950_listing():
    """ppo_values_head_kernel exists under a name of its own, keeps no private segment (nothing spills) and no LDS."""
    from rollout_host_common import _kernel, _listing
    name, body, scratch, static_lds = _kernel(_listing("ppo_fused"), r"_ZN2mi22ppo_values_head_kernelE")
    assert scratch == 0 and static_lds == 0, (name, scratch, static_lds)
    assert "ds_bpermute_b32" in body and "global_store_dword" in body                # the sample's shuffles and its one store
