"""CPU-only tests of running-return reward scaling (mi_rollout_scale_rewards, RolloutBuffer.set_reward_scaling): the numpy float64 reference of the pass (also
imported by tests/test_t_reward_scaling_gpu.py) against two independent spellings, the C-ABI surface and every argument error (dummy buffers that stay unwritten), the
scratch size, the device-free validation of the settings and of a checkpointed state, the pinned signatures and documents, and the gfx950 code of ppo_ops.hip (compiled
here, no GPU needed): the four new kernels exist under names of their own, use no private segment and no static LDS, and the finish kernels keep their names."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

from rollout_host_common import ROOT, _kernel, _listing

D, CD = "double*", "const double*"
SCALE_PROTO = ("int", [("void*", "stream"), (CD, "rewards"), (CD, "terminals"), ("const unsigned char*", "truncs"), ("const int*", "len"), ("int", "num_envs"),
                       ("int", "T"), ("double", "gamma"), ("double", "epsilon"), ("double", "clip"), ("int", "merge"), (D, "state"), (D, "carry"), (D, "scratch"),
                       (D, "g_out"), (D, "rewards_out")])


# ---- the reference: a plain per-lane loop over the formulas of include/mi355_carla.h, numpy float64 ----
def reference(r, d, truncs, lens, gamma, epsilon, clip, merge, state, carry):
    """-> (G [E, T], rewards_out [E, T] (NaN at t >= len), state' float64 [4] = {count, mean, M2, den}, carry' [E]).  The inputs are not changed and entries at
    t >= len are not read."""
    r, d = np.asarray(r, np.float64), np.asarray(d, np.float64)
    E, T = r.shape
    gamma = np.float64(gamma)
    G, out = np.full((E, T), np.nan), np.full((E, T), np.nan)
    carry = np.array(carry, np.float64)
    count, mean, m2 = (np.float64(x) for x in state[:3])
    L = np.minimum(np.asarray(lens, np.int64), T)
    for e in range(E):
        c = carry[e]
        for t in range(L[e]):
            G[e, t] = c * gamma + r[e, t]                                            # one multiply, one add, both rounded to float64
            c = np.float64(0.0) if (d[e, t] != 0 or (truncs is not None and truncs[e, t])) else G[e, t]
        if L[e] >= 1:
            carry[e] = c
    rec = np.arange(T)[None, :] < L[:, None]
    n_b = np.float64(rec.sum())
    if merge and n_b >= 1:
        m_b = G[rec].sum() / n_b
        m2_b = ((G[rec] - m_b) ** 2).sum()
        delta, n_new = m_b - mean, count + n_b
        mean = mean + delta * n_b / n_new
        m2 = m2 + (m2_b + delta * delta * count * n_b / n_new)
        count = n_new
    var = m2 / count if count > 0 else np.float64(1.0)
    den = np.sqrt(var + np.float64(epsilon))
    out[rec] = np.clip(r[rec] / den, -clip, clip)
    return G, out, np.array([count, mean, m2, den], np.float64), carry


def scalar_loop(r, d, truncs, lens, gamma, epsilon, clip, merge, state, carry):
    """The same pass with Python floats only (IEEE doubles, no numpy arithmetic): one list of every recorded G, plain sums in recording order."""
    E, T = len(r), len(r[0])
    count, mean, m2 = float(state[0]), float(state[1]), float(state[2])
    carry = [float(x) for x in carry]
    G = [[None] * T for _ in range(E)]
    flat = []
    for e in range(E):
        n = min(int(lens[e]), T)
        c = carry[e]
        for t in range(n):
            g = c * float(gamma)
            g = g + float(r[e][t])
            G[e][t] = g
            flat.append(g)
            c = 0.0 if (float(d[e][t]) != 0.0 or (truncs is not None and bool(truncs[e][t]))) else g
        if n:
            carry[e] = c
    if merge and flat:
        n_b = float(len(flat))
        m_b = sum(flat) / n_b
        m2_b = sum((g - m_b) * (g - m_b) for g in flat)
        delta = m_b - mean
        n_new = count + n_b
        mean += delta * n_b / n_new
        m2 += m2_b + delta * delta * count * n_b / n_new
        count = n_new
    den = math.sqrt((m2 / count if count > 0 else 1.0) + float(epsilon))
    out = [[None if G[e][t] is None else min(max(float(r[e][t]) / den, -clip), clip) for t in range(T)] for e in range(E)]
    return G, out, [count, mean, m2, den], carry


def make_case(seed, E, T, lens=None, with_truncs=True):
    """A seeded collection: rewards around 2 with a spread of 3 (variance well above 1e-2 mean^2), terminals in the middle of lanes and at a last step, truncations."""
    rng = np.random.RandomState(seed)
    r = 2.0 + 3.0 * rng.standard_normal((E, T))
    d = (rng.uniform(size=(E, T)) < 0.15).astype(np.float64)
    tr = (rng.uniform(size=(E, T)) < 0.1) & (d == 0) if with_truncs else None
    lens = np.asarray(rng.randint(0, T + 1, E) if lens is None else lens, np.int32)
    return r, d, tr, lens


def rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


def test_reference_against_a_scalar_python_loop():
    for seed, E, T, lens in ((1, 1, 1, [1]), (2, 3, 5, [0, 5, 3]), (3, 5, 70, [70, 0, 1, 64, 65]), (4, 70, 3, None)):
        r, d, tr, lens = make_case(seed, E, T, lens)
        carry = np.random.RandomState(seed + 100).standard_normal(E)
        for truncs in (None, tr):
            for merge, state in ((1, np.zeros(4)), (1, np.array([40.0, 1.5, 300.0, 0.0])), (0, np.array([40.0, 1.5, 300.0, 0.0])), (0, np.zeros(4))):
                G, out, st, c = reference(r, d, truncs, lens, 0.99, 1e-8, 1.5, merge, state, carry)
                G2, out2, st2, c2 = scalar_loop(r.tolist(), d.tolist(), None if truncs is None else truncs.tolist(), lens.tolist(), 0.99, 1e-8, 1.5, merge, state, carry)
                for e in range(E):
                    n = min(int(lens[e]), T)
                    assert np.all(np.isnan(G[e, n:])) and np.all(np.isnan(out[e, n:]))
                    assert G[e, :n].tolist() == G2[e][:n] and all(x is None for x in G2[e][n:]), (seed, e)     # the recurrence bit for bit
                    assert np.allclose(out[e, :n], out2[e][:n], rtol=1e-12, atol=0), (seed, e)
                assert c.tolist() == c2                                              # carries bit for bit (0.0 behind a terminal or truncated last step)
                assert st[0] == st2[0] and all(rel(st[k], st2[k]) < 1e-12 for k in (1, 2, 3)), (seed, merge, st, st2)
                if not merge:
                    assert st[:3].tobytes() == np.asarray(state[:3], np.float64).tobytes()
    # the zero state, frozen: den = sqrt(1 + epsilon); lanes of length 0 keep their carry
    r, d, tr, lens = make_case(2, 3, 5, [0, 5, 3])
    G, out, st, c = reference(r, d, None, lens, 0.99, 1e-8, float("inf"), 0, np.zeros(4), [7.0, 1.0, 2.0])
    assert st[3] == math.sqrt(1.0 + 1e-8) and c[0] == 7.0 and np.array_equal(out[1], r[1] / st[3])


def test_chained_merges_are_the_moments_of_the_concatenation():
    """Three collections through the reference, state and carry handed on: count, mean and M2 / count against np.mean / np.var over every collection's G, to 1e-12."""
    E, T = 6, 37
    state, carry, all_g = np.zeros(4), np.zeros(E), []
    for k in range(3):
        r, d, tr, lens = make_case(20 + k, E, T)
        before = carry
        G, out, state, carry = reference(r, d, tr, lens, 0.99, 1e-8, 10.0, 1, state, carry)
        all_g.append(G[~np.isnan(G)])
        cat = np.concatenate(all_g)
        assert state[0] == cat.size
        assert rel(state[1], np.mean(cat)) < 1e-12 and rel(state[2] / state[0], np.var(cat)) < 1e-12, (k, state)
        assert rel(state[3], np.sqrt(np.var(cat) + 1e-8)) < 1e-12
        for e in np.nonzero(lens)[0]:                                                # the carry crosses collections: a lane's first G continues the one before
            assert G[e, 0] == before[e] * np.float64(0.99) + r[e, 0]
        if k:
            assert np.any(before != 0.0)


def test_entry_points_are_declared_and_exported():
    from mi355 import lib as milib
    protos = milib.parse_header()
    assert protos["mi_rollout_scale_rewards"] == SCALE_PROTO
    assert protos["mi_rollout_scale_rewards_scratch_doubles"] == ("long long", [("int", "num_envs")])
    L = milib.get()
    for name in ("mi_rollout_scale_rewards", "mi_rollout_scale_rewards_scratch_doubles"):
        assert hasattr(L.cdll, name), name
    assert L.mi_abi_version() == 7
    sd = L.mi_rollout_scale_rewards_scratch_doubles                                  # needs no GPU: two partials per lane, and n_b, m_b
    assert [sd(n) for n in (-3, 0, 1, 64, 65, 1024)] == [-1, -1, 4, 130, 132, 2050]
    text = open(milib.HEADER).read()
    i = text.index("long long mi_rollout_scale_rewards_scratch_doubles")
    comment = text[text.rfind("/*", 0, i):i]
    for c in ("VecNormalize", "No engine handle", "{count, mean, M2, den}", "G[e,t] = c * gamma + r[e,t]", "no fused multiply-add", "truncs[e,t]", "carry[e] = c",
              "lane-strided", "no floating-point atomics", "bitwise equal", "delta * n_b / n'", "delta^2 * count * n_b / n'", "merge = 0", "bitwise as they were",
              "count > 0 ? M2 / count : 1.0", "sqrt(var + epsilon)", "min(max(r[e,t] / den, -clip), clip)", "a true division", "not written", "not read", "DEVIATIONS",
              "ONE factor", "count = 1e-4", "2 num_envs + 2", "MI_ROLLOUT_MAX_HORIZON", "MI_ROLLOUT_MAX_ENVS", "+inf is valid", "clamped to T"):
        assert c in comment, c


def test_every_argument_error_before_any_launch():
    """No check needs a device and every one runs before the first launch: the dummy host buffers are never written.  Each message starts with the entry's name."""
    from mi355 import lib as milib
    L = milib.get()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    err = L.cdll.mi_last_error
    fn = L.cdll.mi_rollout_scale_rewards
    dbl = ctypes.c_double

    def call(r=p, d=p, tr=None, ln=p, E=3, T=5, gamma=0.99, eps=1e-8, clip=10.0, merge=1, state=p, carry=p, scratch=p, g=p, out=p):
        return fn(None, r, d, tr, ln, E, T, dbl(gamma), dbl(eps), dbl(clip), merge, state, carry, scratch, g, out)
    me = b"mi_rollout_scale_rewards: "
    for name in ("r", "d", "ln", "state", "carry", "scratch", "g", "out"):           # g_out is required: the later passes read it
        assert call(**{name: None}) == -1 and err().startswith(me + b"missing buffers"), name
    for kw in (dict(E=0), dict(E=-2), dict(T=0), dict(T=-1)):
        assert call(**kw) == -1 and err().startswith(me + b"empty input"), kw
    assert call(T=4097) == -1 and err().startswith(me + b"the horizon exceeds MI_ROLLOUT_MAX_HORIZON")
    assert call(E=1025) == -1 and err().startswith(me + b"num_envs exceeds MI_ROLLOUT_MAX_ENVS")
    for bad in (-0.01, 1.0000001, float("nan"), float("inf")):
        assert call(gamma=bad) == -1 and err().startswith(me + b"gamma"), bad
    for bad in (-1e-12, float("nan"), float("inf"), -float("inf")):
        assert call(eps=bad) == -1 and err().startswith(me + b"epsilon"), bad
    for bad in (0.0, -1.0, float("nan"), -float("inf")):
        assert call(clip=bad) == -1 and err().startswith(me + b"clip"), bad
    for bad in (-1, 2, 7):
        assert call(merge=bad) == -1 and err().startswith(me + b"merge"), bad
    assert call(clip=float("inf"), gamma=0.0, eps=0.0, merge=3) == -1 and err().startswith(me + b"merge")      # +inf, 0 and 0 are valid: the next check answers
    assert call(clip=float("inf"), gamma=1.0, tr=p, merge=-1) == -1 and err().startswith(me + b"merge")
    assert all(x == 0.0 for x in buf)
    with pytest.raises(milib.MiError, match=r"mi_rollout_scale_rewards failed \(-1\): mi_rollout_scale_rewards: missing buffers"):
        L.mi_rollout_scale_rewards(None, None, None, None, None, 3, 5, 0.99, 1e-8, 10.0, 1, None, None, None, None, None)
    # the neighbour keeps its message
    assert L.cdll.mi_rollout_finish(None, None, p, p, p, 3, 5, dbl(0.99), dbl(0.95), p, p, None, None, None) == -1 and err() == b"mi_rollout_finish: missing buffers"


def test_settings_validation_needs_no_buffer():
    from rollout import reward_scaling_settings as settings
    assert settings() == {"clip": 10.0, "epsilon": 1e-8, "frozen": False}
    got = settings(np.float32(2.5), 0, np.bool_(True))
    assert got == {"clip": 2.5, "epsilon": 0.0, "frozen": True} and type(got["clip"]) is float and type(got["epsilon"]) is float and type(got["frozen"]) is bool
    assert settings(float("inf"), 1)["clip"] == float("inf")
    for bad in (0, 0.0, -1.0, float("nan"), -float("inf"), True, "10", [10.0], None):
        with pytest.raises(ValueError, match="who: clip is a positive float"):
            settings(bad, who="who")
    for bad in (-1e-9, float("nan"), float("inf"), True, "0", None):
        with pytest.raises(ValueError, match="set_reward_scaling: epsilon is a finite float >= 0"):
            settings(10.0, bad)
    for bad in (0, 1, None, "no", 0.0):
        with pytest.raises(ValueError, match="frozen is a bool"):
            settings(10.0, 1e-8, bad)


def test_state_validation_needs_no_buffer():
    from rollout import reward_scaling_state_checked as checked
    good = dict(count=12.0, mean=-0.5, m2=3.0, carry=np.array([1.0, -2.0, 0.0]), clip=10.0, epsilon=1e-8, frozen=False)
    got = checked(good, 3)
    assert got["carry"].dtype == np.float64 and got["carry"].tolist() == [1.0, -2.0, 0.0] and got["carry"] is not good["carry"]
    assert {k: got[k] for k in good if k != "carry"} == {k: good[k] for k in good if k != "carry"}
    assert checked(dict(good, count=0, m2=0, carry=[1, 2, 3]), 3)["carry"].tolist() == [1.0, 2.0, 3.0]
    who = "load_reward_scaling_state: "
    for missing in good:
        with pytest.raises(ValueError, match=who + "expected a dict"):
            checked({k: v for k, v in good.items() if k != missing}, 3)
    with pytest.raises(ValueError, match=who + "expected a dict"):
        checked([1, 2, 3], 3)
    for key, bad in (("count", -1.0), ("count", float("nan")), ("count", float("inf")), ("count", "3"), ("mean", float("inf")), ("mean", None), ("m2", -1e-3),
                     ("m2", float("nan")), ("m2", True)):
        with pytest.raises(ValueError, match=who + key + " is a finite float"):
            checked(dict(good, **{key: bad}), 3)
    for n, carry in ((4, good["carry"]), (3, np.zeros((3, 1))), (3, np.zeros(2)), (3, 1.0), (3, np.array(["a", "b", "c"]))):
        with pytest.raises(ValueError, match=who + "carry must hold one number per environment"):
            checked(dict(good, carry=carry), n)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match=who + "carry holds a value that is not finite"):
            checked(dict(good, carry=[0.0, bad, 0.0]), 3)
    with pytest.raises(ValueError, match=who + "clip is a positive float"):
        checked(dict(good, clip=0.0), 3)
    with pytest.raises(ValueError, match=who + "frozen is a bool"):
        checked(dict(good, frozen=1), 3)


def test_signatures_and_documents():
    import rollout
    from rollout import ContinuousRolloutBuffer as C, RolloutBuffer as B
    names = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    defaults = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}      # noqa: E731
    assert names(B.set_reward_scaling) == ["self", "clip", "epsilon", "frozen"] and defaults(B.set_reward_scaling) == dict(clip=10.0, epsilon=1e-8, frozen=False)
    assert names(B.reward_scaling_state) == ["self"] and names(B.load_reward_scaling_state) == ["self", "d"]
    assert names(B.zero_return_carry) == ["self", "env_ids"] and defaults(B.zero_return_carry) == dict(env_ids=None)
    for name in ("set_reward_scaling", "reward_scaling_state", "load_reward_scaling_state", "zero_return_carry", "reset"):
        assert getattr(C, name) is getattr(B, name), name                             # one body for both classes
    # pinned by the older tests, unchanged here
    assert names(B.update) == ["self", "gamma", "lam", "num_epochs", "batch_size", "stage_times"]
    assert names(B.update_with_diagnostics) == names(B.update) + ["target_kl"]
    assert names(C.update) == ["self", "gamma", "lam", "num_epochs", "batch_size", "normalize", "stage_times"]
    assert names(C.update_with_diagnostics) == names(C.update) + ["target_kl"]
    for c in ("set_reward_scaling(clip=10.0, epsilon=1e-8)", "mi_rollout_scale_rewards", "return_rms", "reward_scale_den", "scaled_rewards", "discounted_returns",
              "reward_clip_fraction", "return_carry", "load_reward_scaling_state", "zero_return_carry", "ONE factor", "count 0", "reset()"):
        assert c in rollout.__doc__, c
    assert "scaled" in B.update_with_diagnostics.__doc__.lower() and "explained_variance" in B.update_with_diagnostics.__doc__
    for rel_path, needles in (("DESIGN.md", ("mi_rollout_scale_rewards", "VecNormalize")), ("INTEGRATION.md", ("set_reward_scaling", "load_reward_scaling_state")),
                              ("README.md", ("mi_rollout_scale_rewards",)), ("profiles/r18_reward_scaling.md", ("mi_rollout_scale_rewards", "finish"))):
        text = open(os.path.join(ROOT, rel_path)).read()
        for c in needles:
            assert c in text, (rel_path, c)


MI = r"_ZN2mi"
NEW_KERNELS = [MI + r"26rollout_reward_scan_kernelE", MI + r"25rollout_reward_dev_kernelE", MI + r"27rollout_reward_merge_kernelE", MI + r"27rollout_reward_scale_kernelE"]
OLD_KERNELS = [MI + r"21rollout_finish_kernelE", MI + r"25rollout_finish_seg_kernelILi0EE", MI + r"25rollout_finish_seg_kernelILi1EE",
               MI + r"30rollout_finish_seg_boot_kernelILi0EE", MI + r"30rollout_finish_seg_boot_kernelILi1EE", MI + r"25rollout_seg_reduce_kernelILi0EE",
               MI + r"25rollout_seg_reduce_kernelILi1EE", MI + r"23rollout_seg_norm_kernelILi0EE", MI + r"23rollout_seg_norm_kernelILi1EE"]


def test_the_new_kernels_in_the_gfx950_listing():
    text = _listing("ppo_ops")
    names = set()
    for prefix in NEW_KERNELS:
        name, body, scratch, static_lds = _kernel(text, prefix)
        names.add(name)
        assert scratch == 0, name                                                    # no private segment
        assert static_lds == 0, name                                                 # the scan's rewards and flags live in dynamic LDS sized by T, not by the limit
        assert "atomic" not in body and "v_mfma" not in body, name                   # ordered sums only
    assert len(names) == 4
    scan = _kernel(text, NEW_KERNELS[0])[1]
    assert "v_mul_f64" in scan and "v_add_f64" in scan and "v_fma_f64" not in scan   # G = c * gamma + r: one multiply, one add, never contracted
    assert "ds_write_b64" in scan and "ds_write_b8" in scan                          # rewards and reset flags through LDS
    for prefix in NEW_KERNELS[1:3]:                                                  # the ordered sums: fp64 adds and the wave reduction's cross-lane moves
        body = _kernel(text, prefix)[1]
        assert "v_add_f64" in body, prefix
    assert "v_div_scale_f64" in _kernel(text, NEW_KERNELS[3])[1] and "v_rcp_f64" in _kernel(text, NEW_KERNELS[3])[1]      # r / den is a division (not r * (1 / den) formed once)
    assert "v_div_fixup_f64" in _kernel(text, NEW_KERNELS[3])[1]
    for prefix in OLD_KERNELS:                                                       # the finish kernels keep their names
        _kernel(text, prefix)
