"""CPU-only tests of running observation normalisation (mi_rollout_step_batch_norm / mi_rollout_value_batch_norm / mi_rollout_obs_stats,
RolloutBuffer.set_observation_normalization): the numpy float64 reference of the moments pass and the merge (also imported by
tests/test_v_observation_normalization_gpu.py) against np.mean / np.var over the concatenation of three chained merges, the C-ABI surface and every argument error
(dummy buffers that stay unwritten), the scratch size, the device-free validation of the settings and of a checkpointed state, the signatures, normalize_observations
on hand-made cases, the gfx950 code (compiled here, no GPU needed), and -- with a stub library that records entry names -- which entries step / bootstrap / truncate
call with the setting off and on."""
import ctypes
import inspect
import os
import types

import numpy as np
import pytest

from rollout_host_common import ROOT, _kernel, _listing

F, CF, D = "float*", "const float*", "double*"
BATCH = [("void*", "vae_h"), ("void*", "ppo_h"), ("void*", "stream"), ("const unsigned char*", "frames_u8"), (CF, "measurements"), ("int", "n_meas"), (CF, "noise"),
         ("int", "greedy"), ("int", "n"), ("void*", "scratch"), ("long long", "scratch_bytes"), (F, "out")]
VALUE = [a for a in BATCH if a[1] not in ("noise", "greedy")]
NORM = [(CF, "obs_mean"), (CF, "obs_inv_std"), ("float", "obs_clip"), (F, "nstate"), ("const int*", "table_rows"), ("long long", "n_table_rows")]
STEP_NORM_PROTO = ("int", BATCH + NORM + [(F, "tab_states"), (F, "tab_raw_states"), (F, "tab_actions"), (F, "tab_values")])
VALUE_NORM_PROTO = ("int", VALUE + NORM + [(F, "tab_final_values")])
STATS_PROTO = ("int", [("void*", "stream"), (CF, "tab_raw_states"), ("long long", "n_table_rows"), ("const int*", "row_idx"), ("long long", "n"), ("int", "din"),
                       ("int", "first_col"), ("int", "merge"), ("double", "epsilon"), ("float", "clip"), (D, "state"), (F, "obs_mean"), (F, "obs_inv_std"), (D, "scratch"),
                       (D, "batch_out")])


# ---- the reference: the formulas of include/mi355_carla.h in numpy float64 ----
def derive(state, din, epsilon, first_col):
    """-> (mean32, inv32) float32 [din] from state = {count, mean[din], M2[din]}."""
    count, mean, m2 = state[0], state[1:1 + din], state[1 + din:]
    var = m2 / count if count > 0 else np.ones(din)
    mean32, inv32 = mean.astype(np.float32), (np.float64(1.0) / np.sqrt(var + np.float64(epsilon))).astype(np.float32)
    mean32[:first_col], inv32[:first_col] = 0.0, 1.0
    return mean32, inv32


def reference(x, state, merge, epsilon=1e-8, first_col=0):
    """x: float32 [n, din], the rows the list names inside the table; state: float64 [1 + 2 din].  -> (state', mean32, inv32, batch mean, batch M2); `state` is not
    changed."""
    x = np.asarray(x, np.float32).astype(np.float64)
    n, din = x.shape
    state = np.array(state, np.float64)
    m_b = x.sum(0) / n if n else np.zeros(din)
    m2_b = ((x - m_b) ** 2).sum(0) if n else np.zeros(din)
    if merge and n:
        count, mean, m2 = state[0], state[1:1 + din].copy(), state[1 + din:].copy()
        delta, n_new = m_b - mean, count + n
        state[1:1 + din] = mean + delta * n / n_new
        state[1 + din:] = m2 + (m2_b + delta * delta * count * n / n_new)
        state[0] = n_new
    return (state,) + derive(state, din, epsilon, first_col) + (m_b, m2_b)


def columns(rng, n, din):
    """float32 [n, din]: column means N(0, 0.1) and variances in [0.25, 4]; the last column is a speed (mean 15, var 75); column 1 is constant."""
    x = rng.standard_normal((n, din)) * np.sqrt(rng.uniform(0.25, 4.0, din)) + 0.1 * rng.standard_normal(din)
    x[:, -1] = 15.0 + np.sqrt(75.0) * rng.standard_normal(n)
    if din > 1:
        x[:, 1] = 0.375
    return x.astype(np.float32)


def check_moments(state, rows, tag):
    """count exact; mean within 1e-12 max|x| of the column, M2 / count within 1e-9 relative of np.var (at most 1000 fp64 terms: n 2^-53 ~ 1e-13)."""
    rows = np.asarray(rows, np.float32).astype(np.float64)
    n, din = rows.shape
    assert state[0] == n, tag
    mean, var = state[1:1 + din], state[1 + din:] / state[0]
    assert np.all(np.abs(mean - rows.mean(0)) <= 1e-12 * np.abs(rows).max(0)), (tag, np.abs(mean - rows.mean(0)).max())
    ref = rows.var(0)
    assert np.all(np.abs(var - ref) <= 1e-9 * ref), (tag, (np.abs(var - ref) / np.maximum(ref, 1e-300)).max())


def test_reference_chained_merges_are_the_moments_of_the_concatenation():
    for din, sizes in ((67, (5, 257, 1)), (5, (1000, 1, 333)), (100, (300, 300, 300))):
        rng = np.random.RandomState(din)
        state, seen = np.zeros(1 + 2 * din), []
        for k, n in enumerate(sizes):
            x = columns(rng, n, din)
            before = state.copy()
            frozen = reference(x, state, 0)
            assert frozen[0].tobytes() == before.tobytes()                           # merge = 0 leaves the state bitwise
            state, mean32, inv32, m_b, m2_b = reference(x, state, 1)
            seen.append(x)
            check_moments(state, np.concatenate(seen), (din, k))
            if din > 1:
                assert state[1 + din + 1] == 0.0 and state[2] == np.float64(np.float32(0.375))      # the constant column: exact sums, M2 == 0.0
            want = (1.0 / np.sqrt(state[1 + din:] / state[0] + 1e-8)).astype(np.float32)
            assert np.array_equal(inv32, want) and np.array_equal(mean32, state[1:1 + din].astype(np.float32))
        assert reference(np.zeros((0, din), np.float32), state, 1)[0].tobytes() == state.tobytes()      # an empty batch merges nothing
    fresh = reference(np.zeros((0, 4), np.float32), np.zeros(9), 1)
    assert fresh[1].tolist() == [0.0] * 4 and fresh[2].tolist() == [1.0] * 4 and np.float32(1.0 / np.sqrt(1.0 + 1e-8)) == np.float32(1.0)
    off = reference(columns(np.random.RandomState(3), 50, 6), np.zeros(13), 1, first_col=4)
    assert off[1][:4].tolist() == [0.0] * 4 and off[2][:4].tolist() == [1.0] * 4 and np.all(off[2][4:] != 1.0) and np.all(off[0][1 + 6:] >= 0)


def test_entry_points_are_declared_and_exported():
    from mi355 import lib as milib
    protos = milib.parse_header()
    assert protos["mi_rollout_step_batch_norm"] == STEP_NORM_PROTO
    assert protos["mi_rollout_value_batch_norm"] == VALUE_NORM_PROTO
    assert protos["mi_rollout_obs_stats"] == STATS_PROTO
    assert protos["mi_rollout_obs_stats_scratch_doubles"] == ("long long", [("long long", "n"), ("int", "din")])
    assert protos["mi_rollout_step_batch"] == ("int", BATCH) and protos["mi_rollout_value_batch_rec"][1][:len(VALUE)] == VALUE      # "the arguments of" the older entries
    L = milib.get()
    for name in ("mi_rollout_step_batch_norm", "mi_rollout_value_batch_norm", "mi_rollout_obs_stats", "mi_rollout_obs_stats_scratch_doubles"):
        assert hasattr(L.cdll, name), name
    assert L.mi_abi_version() == 7
    text = open(milib.HEADER).read()
    i = text.index("int mi_rollout_step_batch_norm")
    comment = text[text.rfind("/*", 0, i):i]
    for c in ("VecNormalize", "vae_common.py:45-61", "ppo.py:231-251", "one subtract, one multiply", "does not grow", "RAW z", "records nothing",
              "16-byte", "+inf is valid"):
        assert c in comment, c
    i = text.index("long long mi_rollout_obs_stats_scratch_doubles")
    comment = text[text.rfind("/*", 0, i):i]
    for c in ("No engine handle", "{count, mean[din], M2[din]}", "skipped and does not count", "function of n alone", "floating-point atomics",
              "bitwise equal", "delta * n_b / n'", "delta^2 * count * n_b / n'", "bitwise as it was", "count > 0 ? M2 / count : 1.0", "float32(1 / sqrt(var + epsilon))",
              "first_col", "AS THEY WERE ON ENTRY", "DEVIATIONS", "count = 1e-4", "3 nb din + nb + din + 1"):
        assert c in comment, c


def test_scratch_size_needs_no_gpu():
    from mi355 import lib as milib
    sd = milib.get().mi_rollout_obs_stats_scratch_doubles
    assert [sd(n, 67) for n in (-1, 0)] == [-1, -1] and sd(5, 0) == -1 and sd(5, -2) == -1

    def want(n, din):
        chunk = max(32, -(-n // 256))
        nb = -(-n // chunk)
        return 3 * nb * din + nb + din + 1
    for n, din in ((1, 67), (5, 67), (32, 67), (33, 67), (257, 67), (1000, 5), (300, 100), (1024, 128), (8192, 67), (8193, 67), (1024 * 4097, 67)):
        assert sd(n, din) == want(n, din), (n, din)
    assert sd(1, 1) == 6 and sd(33, 2) == 17


def test_every_argument_error_before_any_launch():
    """No check needs a device and every one runs before the first launch: the dummy host buffers are never written.  Each message starts with the entry's name."""
    from mi355 import lib as milib
    L = milib.get()
    buf = (ctypes.c_double * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    err = L.cdll.mi_last_error
    dbl, flt = ctypes.c_double, ctypes.c_float

    def stats(tab=p, n_rows=8, idx=p, n=4, din=3, first=0, merge=1, eps=1e-8, clip=10.0, state=p, mean=p, inv=p, scratch=p, out=p):
        return L.cdll.mi_rollout_obs_stats(None, tab, n_rows, idx, n, din, first, merge, dbl(eps), flt(clip), state, mean, inv, scratch, out)
    me = b"mi_rollout_obs_stats: "
    for name in ("tab", "idx", "state", "mean", "inv", "scratch", "out"):
        assert stats(**{name: None}) == -1 and err().startswith(me + b"missing buffers"), name
    for name in ("state", "mean", "inv", "out"):                                     # an empty list needs neither the table, the list nor the scratch -- but these
        assert stats(n=0, tab=None, idx=None, scratch=None, **{name: None}) == -1 and err().startswith(me + b"missing buffers"), name
    assert stats(n=-1) == -1 and err().startswith(me + b"n is the length of the row list")
    for kw in (dict(din=0), dict(din=-3), dict(n_rows=0)):
        assert stats(**kw) == -1 and err().startswith(me + b"empty input"), kw
    for bad in (-1, 4):
        assert stats(first=bad) == -1 and err().startswith(me + b"first_col"), bad
    for bad in (-1, 2):
        assert stats(merge=bad) == -1 and err().startswith(me + b"merge"), bad
    for bad in (-1e-12, float("nan"), float("inf")):
        assert stats(eps=bad) == -1 and err().startswith(me + b"epsilon"), bad
    for bad in (0.0, -1.0, float("nan"), -float("inf")):
        assert stats(clip=bad) == -1 and err().startswith(me + b"clip"), bad
    assert stats(clip=float("inf"), eps=0.0, first=3, merge=7) == -1 and err().startswith(me + b"merge")      # +inf, 0 and first_col = din are valid: the next check answers

    def step(vae=p, ppo=p, frames=p, meas=p, noise=None, greedy=1, n=4, scratch=p, out=p, mean=p, inv=p, clip=10.0, nstate=p, rows=p, n_rows=8, ts=p, tr=p, ta=p, tv=p):
        return L.cdll.mi_rollout_step_batch_norm(vae, ppo, None, frames, meas, 3, noise, greedy, n, scratch, 0, out, mean, inv, flt(clip), nstate, rows, n_rows, ts, tr, ta, tv)
    me = b"mi_rollout_step_batch_norm: "
    for h in ("vae", "ppo"):
        assert step(**{h: None}) == -4 and err() == me + b"null handle", h
    for name in ("mean", "inv", "nstate"):
        assert step(**{name: None}) == -1 and err().startswith(me + b"missing obs_mean / obs_inv_std / nstate"), name
    assert step(nstate=odd) == -1 and err().startswith(me + b"nstate must be 16-byte aligned")
    for bad in (0.0, -2.0, float("nan")):
        assert step(clip=bad) == -1 and err().startswith(me + b"obs_clip"), bad
    for kw in (dict(ts=None), dict(tr=None), dict(ta=None), dict(tv=None), dict(n_rows=0)):
        assert step(**kw) == -1 and err() == me + b"missing tables", kw
    assert step(frames=None) == -1 and err() == me + b"missing buffers"             # the checks of the entry it extends, under the name of the entry that was called
    assert step(greedy=0) == -1 and err() == me + b"missing buffers"                # sampling without noise
    # the evaluation step (table_rows NULL) reads no table: the call gets as far as the range of n
    assert step(rows=None, ts=None, tr=None, ta=None, tv=None, n=0, clip=float("inf")) == -1 and err().startswith(me + b"1 <= n <= MI_ROLLOUT_MAX_ENVS")

    def value(vae=p, ppo=p, frames=p, meas=p, n=4, scratch=p, out=p, mean=p, inv=p, clip=10.0, nstate=p, rows=p, n_rows=8, tf=p):
        return L.cdll.mi_rollout_value_batch_norm(vae, ppo, None, frames, meas, 3, n, scratch, 0, out, mean, inv, flt(clip), nstate, rows, n_rows, tf)
    me = b"mi_rollout_value_batch_norm: "
    for h in ("vae", "ppo"):
        assert value(**{h: None}) == -4 and err() == me + b"null handle", h
    for name in ("mean", "inv", "nstate"):
        assert value(**{name: None}) == -1 and err().startswith(me + b"missing obs_mean / obs_inv_std / nstate"), name
    assert value(nstate=odd) == -1 and err().startswith(me + b"nstate must be 16-byte aligned")
    for bad in (0.0, float("nan")):
        assert value(clip=bad) == -1 and err().startswith(me + b"obs_clip"), bad
    for kw in (dict(rows=None), dict(tf=None), dict(n_rows=0)):
        assert value(**kw) == -1 and err() == me + b"missing tables", kw
    assert value(n=1025) == -1 and err().startswith(me + b"1 <= n <= MI_ROLLOUT_MAX_ENVS")
    assert all(x == 0.0 for x in buf)
    with pytest.raises(milib.MiError, match=r"mi_rollout_obs_stats failed \(-1\): mi_rollout_obs_stats: missing buffers"):
        L.mi_rollout_obs_stats(None, None, 8, None, 4, 3, 0, 1, 1e-8, 10.0, None, None, None, None, None)
    # the neighbours keep their messages
    assert L.cdll.mi_rollout_step_batch_rec(p, p, None, p, p, 3, None, 1, 4, p, 0, p, None, 8, p, p, p) == -1 and err() == b"mi_rollout_step_batch_rec: missing tables"
    assert L.cdll.mi_rollout_value_batch_rec(p, p, None, p, p, 3, 4, p, 0, p, None, 8, p) == -1 and err() == b"mi_rollout_value_batch_rec: missing tables"
    assert L.cdll.mi_rollout_value_batch_rec(p, p, None, None, p, 3, 4, p, 0, p, p, 8, p) == -1 and err() == b"mi_rollout_value_batch_rec: missing buffers"
    assert L.cdll.mi_rollout_step_batch(p, p, None, None, p, 3, None, 1, 4, p, 0, p) == -1 and err() == b"mi_rollout_step_batch: missing buffers"


def test_settings_validation_needs_no_buffer():
    from rollout import observation_normalization_settings as settings
    assert settings() == {"clip": 10.0, "epsilon": 1e-8, "frozen": False, "normalize_latents": True}
    got = settings(np.float32(2.5), 0, np.bool_(True), np.bool_(False))
    assert got == {"clip": 2.5, "epsilon": 0.0, "frozen": True, "normalize_latents": False}
    assert [type(got[k]) for k in ("clip", "epsilon", "frozen", "normalize_latents")] == [float, float, bool, bool]
    assert settings(float("inf"))["clip"] == float("inf")
    for bad in (0, 0.0, -1.0, float("nan"), -float("inf"), True, "10", [10.0], None):
        with pytest.raises(ValueError, match="who: clip is a positive float"):
            settings(bad, who="who")
    for bad in (-1e-9, float("nan"), float("inf"), True, "0", None):
        with pytest.raises(ValueError, match="set_observation_normalization: epsilon is a finite float >= 0"):
            settings(10.0, bad)
    for bad in (0, 1, None, "no"):
        with pytest.raises(ValueError, match="frozen is a bool"):
            settings(10.0, 1e-8, bad)
        with pytest.raises(ValueError, match="normalize_latents is a bool"):
            settings(10.0, 1e-8, False, bad)


GOOD = dict(count=12.0, mean=np.array([1.0, -2.0, 0.0]), m2=np.array([3.0, 0.0, 48.0]), z_dim=2, clip=10.0, epsilon=1e-8, frozen=False, normalize_latents=True)


def test_state_validation_needs_no_buffer():
    from rollout import observation_normalization_state_checked as checked
    got = checked(GOOD, 3)
    for k in ("mean", "m2"):
        assert got[k].dtype == np.float64 and got[k].tolist() == GOOD[k].tolist() and got[k] is not GOOD[k]
    assert {k: got[k] for k in GOOD if k not in ("mean", "m2")} == {k: GOOD[k] for k in GOOD if k not in ("mean", "m2")}
    assert checked(dict(GOOD, count=0, mean=[0, 0, 0], m2=[0, 0, 0], z_dim=np.int64(3)), 3)["z_dim"] == 3
    who = "load_observation_normalization_state: "
    for missing in GOOD:
        with pytest.raises(ValueError, match=who + "expected a dict"):
            checked({k: v for k, v in GOOD.items() if k != missing}, 3)
    with pytest.raises(ValueError, match=who + "expected a dict"):
        checked([1, 2, 3], 3)
    for bad in (-1.0, float("nan"), float("inf"), "3", True):
        with pytest.raises(ValueError, match=who + "count is a finite float >= 0"):
            checked(dict(GOOD, count=bad), 3)
    for bad in (-1, 4, 2.0, True, None):
        with pytest.raises(ValueError, match=who + "z_dim is an int"):
            checked(dict(GOOD, z_dim=bad), 3)
    for key in ("mean", "m2"):
        for din, bad in ((3, np.zeros(4)), (3, np.zeros((3, 1))), (3, np.zeros(2)), (3, 1.0), (3, np.array(["a", "b", "c"]))):
            with pytest.raises(ValueError, match=who + key + " must hold one number per observation column"):
                checked(dict(GOOD, **{key: bad}), din)
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError, match=who + key + " holds a value that is not finite"):
                checked(dict(GOOD, **{key: [0.0, bad, 0.0]}), 3)
    with pytest.raises(ValueError, match=who + r"mean must hold one number per observation column, shape \(4,\)"):
        checked(GOOD, 4)                                                             # a state of another input size
    with pytest.raises(ValueError, match=who + "m2 holds a value that is not finite or is negative"):
        checked(dict(GOOD, m2=[0.0, -1e-9, 0.0]), 3)
    with pytest.raises(ValueError, match=who + "clip is a positive float"):
        checked(dict(GOOD, clip=0.0), 3)
    with pytest.raises(ValueError, match=who + "normalize_latents is a bool"):
        checked(dict(GOOD, normalize_latents=1), 3)


def test_normalize_observations_on_hand_made_cases():
    from rollout import normalize_observations as norm
    fresh = dict(GOOD, count=0.0, mean=np.zeros(3), m2=np.zeros(3))
    x = np.array([[0.5, -3.25, 9.75], [1e-3, 0.0, -10.0]])
    got = norm(x, fresh)
    assert got.dtype == np.float32 and got.shape == x.shape and np.array_equal(got, x.astype(np.float32))      # count 0: the identity ...
    assert norm(np.array([11.0, -30.0, 10.0]), fresh).tolist() == [10.0, -10.0, 10.0]                        # ... apart from the clamp
    assert np.array_equal(norm(np.array([11.0, -30.0, 1e30]), dict(fresh, clip=float("inf"))), np.array([11.0, -30.0, 1e30], np.float32))
    # mean 1 / var 0.25, a constant column at -2 (var 0: inv = 1 / sqrt(1e-8) = 1e4), mean 0 / var 4
    got = norm(np.array([[2.0, -2.0, 3.0], [1.0, -2.0, -50.0], [0.5, -1.0, 20.0]]), GOOD)
    assert got[:, 1].tolist() == [0.0, 0.0, 10.0]                                    # the constant column gives 0.0; a value off it is blown up to +clip
    assert got[1].tolist() == [0.0, 0.0, -10.0] and got[2, 2] == 10.0                # a clamped entry is exactly +-clip
    inv0 = np.float32(1.0 / np.sqrt(0.25 + 1e-8))
    assert got[0, 0] == (np.float32(2.0) - np.float32(1.0)) * inv0 and got[2, 0] == np.float32(-0.5) * inv0
    assert got[0, 2] == np.float32(3.0) * np.float32(1.0 / np.sqrt(4.0 + 1e-8))
    # normalize_latents = False leaves the first z_dim columns alone (the clamp still applies to them)
    got = norm(np.array([[2.0, -2.0, 3.0], [12.0, -1.0, 3.0]]), dict(GOOD, normalize_latents=False))
    assert got[:, :2].tolist() == [[2.0, -2.0], [10.0, -1.0]] and got[0, 2] == np.float32(3.0) * np.float32(1.0 / np.sqrt(4.0 + 1e-8))
    assert norm(np.array([0.1], np.float64), dict(GOOD, count=0.0, mean=[0.0], m2=[0.0], z_dim=0, clip=0.05))[0] == np.float32(0.05)      # clip itself is rounded to float32
    with pytest.raises(ValueError, match="normalize_observations: mean must hold one number per observation column"):
        norm(np.zeros((2, 4)), GOOD)


def test_signatures_and_documents():
    import rollout
    from rollout import BatchedRolloutStep as S, ContinuousRolloutBuffer as C, RolloutBuffer as B, RolloutStep as R
    names = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    defaults = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}      # noqa: E731
    assert names(B.set_observation_normalization) == ["self", "clip", "epsilon", "frozen", "normalize_latents"]
    assert defaults(B.set_observation_normalization) == dict(clip=10.0, epsilon=1e-8, frozen=False, normalize_latents=True)
    assert names(B.observation_normalization_state) == ["self"] and names(B.load_observation_normalization_state) == ["self", "d"]
    assert names(B.merge_observation_statistics) == ["self"]
    for name in ("set_observation_normalization", "observation_normalization_state", "load_observation_normalization_state", "merge_observation_statistics", "step"):
        assert getattr(C, name) is getattr(B, name), name                             # one body for both classes
    assert names(S.set_observation_normalization) == ["self", "state_dict"] and names(R.set_observation_normalization) == ["self", "state_dict"]
    assert names(rollout.normalize_observations) == ["states", "state_dict"]
    # pinned by the older tests, unchanged here
    assert names(B.update) == ["self", "gamma", "lam", "num_epochs", "batch_size", "stage_times"]
    assert names(C.update) == ["self", "gamma", "lam", "num_epochs", "batch_size", "normalize", "stage_times"]
    assert names(B.step) == ["self", "frames_u8", "measurements", "env_ids", "greedy", "noise"] and names(C.truncate) == ["self", "final_frames_u8", "final_measurements", "env_ids"]
    r = object.__new__(R)
    r.set_observation_normalization(None)
    with pytest.raises(ValueError, match=r"BatchedRolloutStep\(vae, ppo, num_envs=1\)"):
        r.set_observation_normalization(dict(GOOD))
    for c in ("set_observation_normalization(clip=10.0, epsilon=1e-8)", "mi_rollout_step_batch_norm", "mi_rollout_value_batch_norm", "mi_rollout_obs_stats",
              "rollout_obs_norm_kernel", "raw_states", "observation_rms", "observation_clip_fraction", "observation_stats", "merge_observation_statistics",
              "load_observation_normalization_state", "normalize_observations", "normalize_latents=False", "ONE set of statistics", "count 0", "VecNormalize",
              "BatchedRolloutStep(num_envs=1)"):
        assert c in rollout.__doc__, c
    assert "observation_rms" in B.update.__doc__ and "observation_clip_fraction" in B.update.__doc__
    for rel_path, needles in (("DESIGN.md", ("mi_rollout_obs_stats", "rollout_obs_norm_kernel")), ("INTEGRATION.md", ("set_observation_normalization", "normalize_observations")),
                              ("README.md", ("mi_rollout_step_batch_norm", "mi_rollout_obs_stats")),
                              ("profiles/r20_observation_normalization.md", ("mi_rollout_obs_stats", "rollout_latency.py"))):
        text = open(os.path.join(ROOT, rel_path)).read()
        for c in needles:
            assert c in text, (rel_path, c)


MI = r"_ZN2mi"
NORM_KERNEL = MI + r"23rollout_obs_norm_kernelE"
STATS_KERNELS = [MI + r"22rollout_obs_sum_kernelE", MI + r"22rollout_obs_dev_kernelE", MI + r"24rollout_obs_merge_kernelE"]


def test_the_new_kernels_in_the_gfx950_listing():
    import test_reward_scaling_host as rs
    import test_rollout_buffer_host as rb
    text = _listing("rollout")
    name, body, scratch, static_lds = _kernel(text, NORM_KERNEL)
    assert scratch == 0 and static_lds == 0, name                                    # no private segment
    assert "v_mfma" not in body and "atomic" not in body, name
    assert "v_sub_f32" in body and "v_mul_f32" in body and "v_fma_f32" not in body and "v_mad_f32" not in body, name      # one subtract, one multiply, never contracted
    assert "global_store_dword" in body, name                                        # nstate and the table row leave through the vector unit
    for prefix in rb.HEADS_REC + rb.EXISTING:                                        # every kernel the older test lists keeps its name
        _kernel(text, prefix)
    text = _listing("ppo_ops")
    names = set()
    for prefix in STATS_KERNELS:
        name, body, scratch, static_lds = _kernel(text, prefix)
        names.add(name)
        assert scratch == 0 and static_lds == 0, name
        assert "atomic" not in body and "v_mfma" not in body, name                   # ordered sums only
        assert "v_add_f64" in body, name
    assert len(names) == 3
    body = _kernel(text, STATS_KERNELS[0])[1]
    assert "v_cvt_f64_f32" in body and "v_sub_f32" in body and "v_fma_f64" not in body and "v_fma_f32" not in body      # fp64 sums of fp32 rows; the step's fp32 expression
    assert "v_mul_f64" in _kernel(text, STATS_KERNELS[1])[1]                         # (x - m_b)^2: a product and an add, not contracted into the sum
    merge = _kernel(text, STATS_KERNELS[2])[1]
    assert "v_cvt_f32_f64" in merge and "v_div_scale_f64" in merge                   # M2 / count and 1 / sqrt(..) are divisions; the fp32 pair is rounded once
    for prefix in [rb.FINISH] + rs.NEW_KERNELS + rs.OLD_KERNELS:
        _kernel(text, prefix)


# ---- which entries the buffers call: a stub library that records names, CPU tensors in place of the pinned / device ones ----
class StubLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("mi_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, len(args)))
            return 0
        return entry


def stub_buffer(monkeypatch, E=3, T=4):
    import torch
    import rollout
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0, synchronize=lambda: None))
    s = object.__new__(rollout._RecordingStep)
    s.L, s.num_envs, s.z_dim, s.A, s.n_meas, s.frame_bytes, s.io, s.device = StubLib(), E, 4, 2, 3, 12, "pinned", "cpu"
    s._rng, s._obs_norm, s.row = np.random.Generator(np.random.Philox(1)), None, 2 + 1 + 4
    s._f_off = (E * s.frame_bytes + 15) // 16 * 16
    s.h_in, s.h_out = torch.zeros(s._f_off + 4 * E * (s.n_meas + s.A + 1), dtype=torch.uint8), torch.zeros(E * s.row)
    s.d_in = s.d_out = None
    s._in_np = s.h_in.numpy()
    s._f_np, s._i_np = s._in_np[s._f_off:].view(np.float32), s._in_np[s._f_off:].view(np.int32)
    s._out_np = s.h_out.numpy().reshape(E, s.row)
    s.scratch, s.scratch_bytes = torch.zeros(16, dtype=torch.uint8), 16
    s.vae = s.ppo = types.SimpleNamespace(dev=types.SimpleNamespace(handle=1))
    b = object.__new__(rollout.ContinuousRolloutBuffer)
    b.rows, b._step, b.L, b.device, b.num_envs, b.horizon, b.n_table_rows = rollout.SegmentedRows(E, T), s, s.L, "cpu", E, T, E * (T + 1)
    b.states, b.actions = torch.zeros(b.n_table_rows, 7), torch.zeros(b.n_table_rows, 2)
    b.values, b.final_values = torch.zeros(b.n_table_rows), torch.zeros(b.n_table_rows)
    b._obs_norm = b.raw_states = None
    return b, s


def collect(b, E):
    frames, meas = np.zeros((E, 2, 2, 3), np.uint8), np.zeros((E, 3))
    b.rows.reset()
    b.step(frames, meas)
    b.outcome(np.zeros(E), np.zeros(E, bool))
    b.truncate(frames[:1], meas[:1], env_ids=[0])
    b.bootstrap(frames[1:], meas[1:], env_ids=np.arange(1, E))


def test_which_entries_step_bootstrap_and_truncate_call(monkeypatch):
    import torch
    import rollout
    b, s = stub_buffer(monkeypatch)
    collect(b, 3)
    assert s.L.calls == [("mi_rollout_step_batch_rec", 17), ("mi_rollout_value_batch_rec", 13), ("mi_rollout_step_batch_rec", 17)]      # off: the entries of today
    del s.L.calls[:]
    s(np.zeros((2, 2, 2, 3), np.uint8), np.zeros((2, 3)), greedy=True)
    assert s.L.calls == [("mi_rollout_step_batch", 12)]
    # on: the _norm entries, with the arguments the header declares
    del s.L.calls[:]
    on = rollout._obs_norm_tensors("cpu", 7, 3)
    on.update(rollout.observation_normalization_settings())
    b._obs_norm = s._obs_norm = on
    b.raw_states = torch.zeros_like(b.states)
    collect(b, 3)
    s(np.zeros((2, 2, 2, 3), np.uint8), np.zeros((2, 3)), greedy=True)
    assert s.L.calls == [("mi_rollout_step_batch_norm", len(STEP_NORM_PROTO[1])), ("mi_rollout_value_batch_norm", len(VALUE_NORM_PROTO[1])),
                         ("mi_rollout_step_batch_norm", len(STEP_NORM_PROTO[1])), ("mi_rollout_step_batch_norm", len(STEP_NORM_PROTO[1]))]
    # turning it on or off with steps recorded is refused before anything changes; off again after reset(): the entries of today
    with pytest.raises(ValueError, match="steps are recorded"):
        b.set_observation_normalization(None)
    with pytest.raises(ValueError, match="steps are recorded"):
        b.load_observation_normalization_state(dict(GOOD, mean=np.zeros(7), m2=np.zeros(7), z_dim=4))
    assert b._obs_norm is on and b.raw_states is not None
    b.reset()
    b.set_observation_normalization(None)
    assert b._obs_norm is None and s._obs_norm is None and b.raw_states is None
    del s.L.calls[:]
    collect(b, 3)
    assert [c[0] for c in s.L.calls] == ["mi_rollout_step_batch_rec", "mi_rollout_value_batch_rec", "mi_rollout_step_batch_rec"]
    for what in ("observation_normalization_state", "merge_observation_statistics"):
        with pytest.raises(ValueError, match="observation normalisation is off"):
            getattr(b, what)()
