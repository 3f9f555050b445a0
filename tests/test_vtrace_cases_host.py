"""The V-trace cases and references on the CPU (tests/vtrace_cases.py): reference (a), the recurrence in the kernel's operation order, is oracle.ppo_oracle's GAE
bit for bit when the policy has not moved, and agrees with reference (b), the forward definition written on its own; no case is degenerate; the settings of
RolloutBuffer.set_vtrace are checked without a device; and the built library exports the two new entries, declared in the header."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "carla-ppo_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import vtrace_cases as vc  # noqa: E402
from oracle import ppo_oracle as po  # noqa: E402

IDS = vc.case_ids()
IDS_IDENTITY = [cid for cid in IDS if min(cid[2]) >= 1.0]                            # the identity is stated for bars >= 1


@pytest.mark.parametrize("cid", IDS_IDENTITY, ids=vc.case_name)
def test_unit_weights_and_bars_of_at_least_one_are_the_oracles_gae(cid):
    """w = 1 with rho_bar >= 1 and c_bar >= 1: D = A = compute_gae on every segment, bitwise, under either successor rule."""
    c = vc.case(cid)
    gl = c["gamma"] * c["lam"]
    for e, s, n, kind in c["segs"]:
        for rbd in (False, True):
            D, A = vc.recurrence(vc.deltas(c, e, s, n, kind, rbd), np.ones(n), gl, c["rho_bar"], c["c_bar"])
            last = s + n - 1
            if kind == vc.TRUNCATED:
                boot = float(c["final_values"][e, last])
            elif not rbd and c["dones"][e, last] != 0.0:
                boot = 0.0
            else:
                boot = float(c["values"][e, last + 1])
            gae = po.compute_gae(c["rewards"][e, s:s + n], c["values"][e, s:s + n].astype(np.float64), boot, c["dones"][e, s:s + n], c["gamma"], c["lam"])
            assert np.array_equal(A, gae) and np.array_equal(D, gae), (cid, e, s, n, rbd)


@pytest.mark.parametrize("cid", IDS, ids=vc.case_name)
def test_the_recurrence_is_the_forward_definition(cid):
    """Within 1e-12 of max(|D|, |A|): fp64 reassociation over at most 70 terms."""
    c = vc.case(cid)
    w = vc.weights64(c)
    worst = 0.0
    for e, s, n, kind in c["segs"]:
        delta = vc.deltas(c, e, s, n, kind, False)
        D, A = vc.recurrence(delta, w[e, s:s + n], c["gamma"] * c["lam"], c["rho_bar"], c["c_bar"])
        D_b, A_b = vc.forward_definition(delta, w[e, s:s + n], c["gamma"], c["lam"], c["rho_bar"], c["c_bar"])
        scale = max(np.abs(D).max(), np.abs(A).max())
        err = max(np.abs(D - D_b).max(), np.abs(A - A_b).max())
        assert err <= 1e-12 * scale, (cid, e, s, n, err, scale)
        worst = max(worst, err / scale)
    print("%s: (a) against (b), worst %.3e of max(|D|, |A|)" % (vc.case_name(cid), worst))


def test_no_case_is_degenerate():
    """Every finite positive bar has an executed step above it and one below it (the one-step shape: over its two variants); the kinds of segment and of bad
    descriptor the cases are meant to carry are there."""
    groups = {}
    for cid in IDS:
        groups.setdefault(cid[:3], []).append(vc.case(cid))
    for key, cases in groups.items():
        for name, (above, below) in vc.both_sides(cases).items():
            bar = cases[0][name]
            assert above, (key, name)
            assert below or bar == 0.0, (key, name)                                 # (no weight lies below a bar of 0)
    for cid in IDS:
        c = vc.case(cid)
        E, T = c["E"], c["T"]
        kinds = {k for *_, k in c["segs"]}
        if E * T > 1:
            assert kinds == {vc.TERMINAL, vc.TRUNCATED, vc.OPEN}, cid
            assert len(c["segs"]) > E                                               # several segments per lane
            assert len({n for _, _, n, _ in c["segs"]}) > 1                         # ragged
            bad_r, bad_n = c["seg_row"][~c["executed"]], c["seg_len"][~c["executed"]]
            assert (bad_n < 1).any() and (bad_r < 0).any() and (bad_r // (T + 1) >= E).any() and ((bad_r % (T + 1) + bad_n > T) & (bad_r >= 0) & (bad_r // (T + 1) < E)).any()
        for e, s, n, _ in c["segs"]:
            assert 0 <= e < E and s >= 0 and n >= 1 and s + n <= T
        taken = np.zeros((E, T), int)
        for e, s, n, _ in c["segs"]:
            taken[e, s:s + n] += 1
        assert taken.max() == 1                                                      # no two segments share a slot


def test_the_normalisation_of_the_reference_is_train_py():
    """The device-ordered sums of reference() against numpy's mean / std: the same quantity up to reassociation."""
    c = vc.case((5, 70, (2.5, 1.5), 0))
    w = vc.weights64(c)
    for normalize in (0, 1):
        ref = vc.reference(c, w, False, normalize)
        if normalize:
            ok = ~np.isnan(ref["raw"])
            want = (ref["raw"][ok] - ref["raw"][ok].mean()) / (ref["raw"][ok].std() + 1e-8)
            assert np.allclose(ref["adv"][ok], want, rtol=1e-12, atol=1e-12)
        else:
            for e, s, n, _ in c["segs"]:
                A = ref["raw"][e, s:s + n]
                assert np.allclose(ref["adv"][e, s:s + n], (A - A.mean()) / (A.std() + 1e-8), rtol=1e-10, atol=1e-12)


def test_set_vtrace_checks_its_arguments():
    import rollout
    assert rollout.vtrace_settings() == {"rho_bar": 1.0, "c_bar": 1.0}
    assert rollout.vtrace_settings(float("inf"), 0) == {"rho_bar": float("inf"), "c_bar": 0.0}
    assert rollout.vtrace_settings(np.float32(2.5), np.float64(1.5)) == {"rho_bar": 2.5, "c_bar": 1.5}
    for bad in (dict(rho_bar=0.0), dict(rho_bar=-1.0), dict(rho_bar=float("nan")), dict(rho_bar=True), dict(rho_bar="1"), dict(c_bar=-0.5), dict(c_bar=float("nan")),
                dict(c_bar=None), dict(c_bar=False)):
        with pytest.raises(ValueError, match="set_vtrace"):
            rollout.vtrace_settings(**bad)


def test_the_library_exports_the_entries_and_the_header_declares_them():
    from mi355 import lib as milib
    import torch  # noqa: F401  (first, as mi355.lib loads it: both bind one HIP runtime)
    protos = milib.parse_header()
    cdll = ctypes.CDLL(milib.LIB_PATH)
    for name, n_args in (("mi_rollout_finish_vtrace", 26), ("mi_ppo_logp_idx", 8)):
        assert name in protos and len(protos[name][1]) == n_args and protos[name][0] == "int", name
        assert hasattr(cdll, name), name
