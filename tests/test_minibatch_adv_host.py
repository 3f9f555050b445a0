"""CPU-only tests of per-minibatch advantage normalisation (mi_ppo_minibatch_advantages, RolloutBuffer.set_minibatch_normalization): the numpy float64 reference of the
pass (also imported by tests/test_u_minibatch_adv_gpu.py) against a second spelling in plain Python floats, the C-ABI surface and every argument error (dummy buffers
that stay unwritten, the message names the argument), the size of the statistics, the device-free validation of the setting and its off state on buffers built without
__init__, the prototypes as the header writes them, the documents, and the gfx950 code of ppo_ops.hip (compiled here, no GPU needed): the new kernel exists under a
name of its own and the finish, reward-scaling and value-clipping kernels keep theirs."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

from rollout_host_common import ROOT, _kernel, _listing

STATS_PROTO = ("long long", [("int", "n"), ("int", "batch_size")])
PASS_PROTO = ("int", [("void*", "stream"), ("const double*", "adv_raw"), ("const int*", "perm"), ("int", "n"), ("int", "batch_size"), ("int", "num_envs"), ("int", "T"),
                      ("int", "ddof"), ("float*", "tab_adv_out"), ("double*", "stats")])


# ---- the reference: the formulas of include/mi355_carla.h minibatch by minibatch, numpy float64 ----
def reference(adv_raw, perm, batch_size, E, T, ddof):
    """-> (table float64 [E (T + 1)]: (a - mean) / (std + 1e-8) at the rows perm names, NaN everywhere else; stats float64 [n_mb, 3] = {count, mean, std}).  An entry
    of perm that names no step slot is skipped; entries of adv_raw that perm does not name are not read."""
    a = np.asarray(adv_raw, np.float64).reshape(E, T)
    perm = np.asarray(perm, np.int64)
    n_mb = -(-perm.shape[0] // batch_size)
    table, stats = np.full(E * (T + 1), np.nan), np.zeros((n_mb, 3))
    for b in range(n_mb):
        rows = perm[b * batch_size:(b + 1) * batch_size]
        rows = rows[(rows >= 0) & (rows < E * (T + 1)) & (rows % (T + 1) != T)]
        c = rows.shape[0]
        if c == 0:
            continue
        x = a[rows // (T + 1), rows % (T + 1)]
        mean = x.sum() / c
        ss = ((x - mean) ** 2).sum()
        std = np.sqrt(ss / (c - ddof)) if c - ddof >= 1 else np.float64(0.0)
        table[rows] = (x - mean) / (std + 1e-8)
        stats[b] = c, mean, std
    return table, stats


def scalar_loop(adv_raw, perm, batch_size, E, T, ddof):
    """The same pass with Python floats and ints only (IEEE doubles, no numpy arithmetic), plain sums in minibatch order -> ({row: value}, [[count, mean, std], ..])."""
    table, stats = {}, []
    for lo in range(0, len(perm), batch_size):
        kept = []
        for row in perm[lo:lo + batch_size]:
            lane, slot = divmod(row, T + 1) if row >= 0 else (-1, 0)
            if 0 <= lane < E and slot < T:
                kept.append((row, float(adv_raw[lane][slot])))
        c = len(kept)
        if c == 0:
            stats.append([0.0, 0.0, 0.0])
            continue
        total = 0.0
        for _, x in kept:
            total += x
        mean = total / c
        ss = 0.0
        for _, x in kept:
            ss += (x - mean) * (x - mean)
        std = math.sqrt(ss / (c - ddof)) if c - ddof >= 1 else 0.0
        for row, x in kept:
            table[row] = (x - mean) / (std + 1e-8)
        stats.append([float(c), mean, std])
    return table, stats


def make_case(E, T, lens, seed):
    """-> (adv_raw float64 [E, T]: 0.3 + 2 N(0, 1) at the recorded steps and NaN beyond a lane's length, perm int32: the recorded steps' table rows, shuffled)."""
    rng = np.random.RandomState(seed)
    lens = np.asarray(lens, np.int64)
    a = 0.3 + 2.0 * rng.standard_normal((E, T))
    a[np.arange(T)[None, :] >= lens[:, None]] = np.nan
    rows = np.concatenate([e * (T + 1) + np.arange(lens[e]) for e in range(E)]).astype(np.int32)
    rng.shuffle(rows)
    return a, rows


# (E, T, batch_size, lengths): the shapes of the GPU test
CASES = [(1, 1, 1, [1]), (3, 5, 4, [5, 2, 0]), (3, 5, 64, [5, 2, 0]), (5, 70, 64, [70] * 5), (5, 70, 65, [70] * 5), (5, 70, 256, [70] * 5), (5, 70, 257, [70] * 5),
         (70, 3, 32, None)]


def case_lengths(E, T, lens, seed):
    if lens is not None:
        return lens
    lens = np.random.RandomState(seed).randint(0, T + 1, E)
    lens[0], lens[1] = T, 0
    return lens.tolist()


def test_reference_against_a_scalar_python_loop():
    for k, (E, T, batch, lens) in enumerate(CASES):
        lens = case_lengths(E, T, lens, 50 + k)
        a, perm = make_case(E, T, lens, k)
        assert perm.shape[0] == sum(lens)
        planted = perm.tolist()
        if len(planted) > 2:                                                         # entries that name no step slot: a bootstrap slot, rows outside the table
            planted[1:1] = [T, -1, E * (T + 1), E * (T + 1) + 3]
        for ddof in (0, 1):
            for p in (perm.tolist(), planted):
                table, stats = reference(a, p, batch, E, T, ddof)
                table2, stats2 = scalar_loop(a.tolist(), p, batch, E, T, ddof)
                assert stats.shape == (-(-len(p) // batch), 3) == np.asarray(stats2).shape
                assert stats[:, 0].tolist() == [s[0] for s in stats2] and stats[:, 0].sum() == perm.shape[0]        # the planted entries do not count
                scale = np.abs(a[~np.isnan(a)]).max()
                assert np.abs(stats[:, 1:] - np.asarray(stats2)[:, 1:]).max() <= 1e-12 * scale
                assert sorted(table2) == sorted(perm.tolist()) == np.nonzero(~np.isnan(table))[0].tolist()          # the rows perm names and no other
                for row, want in table2.items():
                    assert table[row] == pytest.approx(want, rel=1e-9, abs=1e-12), (E, T, batch, ddof, row)
                one = stats[:, 0] == 1
                assert np.all(stats[one, 2] == 0.0)                                  # a one-sample minibatch: std 0 with either ddof, the entry 0.0
                for b in np.nonzero(one)[0]:
                    rows = [r for r in p[b * batch:(b + 1) * batch] if 0 <= r < E * (T + 1) and r % (T + 1) != T]
                    assert table[rows[0]] == 0.0
    # ddof: the same means, std_1 = std_0 sqrt(c / (c - 1))
    a, perm = make_case(5, 70, [70] * 5, 3)
    s0, s1 = reference(a, perm, 64, 5, 70, 0)[1], reference(a, perm, 64, 5, 70, 1)[1]
    assert np.array_equal(s0[:, :2], s1[:, :2])
    assert np.allclose(s1[:, 2], s0[:, 2] * np.sqrt(s0[:, 0] / (s0[:, 0] - 1)), rtol=1e-12, atol=0)
    # against numpy's own mean / std on one minibatch
    x = a.reshape(-1)[:64]
    rows = (np.arange(64) // 70 * 71 + np.arange(64) % 70).astype(np.int32)
    table, stats = reference(a, rows, 64, 5, 70, 1)
    assert stats[0, 1] == pytest.approx(x.mean(), rel=1e-12) and stats[0, 2] == pytest.approx(x.std(ddof=1), rel=1e-12)
    assert np.allclose(table[rows], (x - x.mean()) / (x.std(ddof=1) + 1e-8), rtol=1e-9, atol=1e-12)
    # a minibatch whose entries all name no slot: {0, 0, 0} and nothing stored
    table, stats = reference(a, [70, -5, 141, 9999], 4, 5, 70, 0)
    assert np.array_equal(stats, np.zeros((1, 3))) and np.all(np.isnan(table))


def test_entry_points_are_declared_and_exported():
    from mi355 import lib as milib
    protos = milib.parse_header()
    assert protos["mi_ppo_minibatch_advantages_stats_doubles"] == STATS_PROTO
    assert protos["mi_ppo_minibatch_advantages"] == PASS_PROTO
    text = open(milib.HEADER).read()
    for written in ("long long mi_ppo_minibatch_advantages_stats_doubles(int n, int batch_size);",
                    "int mi_ppo_minibatch_advantages(void* stream, const double* adv_raw, const int* perm, int n, int batch_size, int num_envs, int T, int ddof, "
                    "float* tab_adv_out, double* stats);"):
        assert written in text, written
    L = milib.get()
    for name in ("mi_ppo_minibatch_advantages", "mi_ppo_minibatch_advantages_stats_doubles"):
        assert hasattr(L.cdll, name), name
    assert L.mi_abi_version() == 7                                                   # two entries more, none changed
    sd = L.mi_ppo_minibatch_advantages_stats_doubles                                 # needs no GPU: three doubles per minibatch
    assert [sd(n, b) for n, b in ((1, 1), (17, 4), (16, 4), (7, 64), (350, 256), (350, 257), (131072, 32), (2 ** 31 - 1, 1), (2 ** 31 - 1, 2 ** 31 - 1))] == \
        [3, 15, 12, 3, 6, 6, 12288, 3 * (2 ** 31 - 1), 3]
    assert [sd(n, b) for n, b in ((0, 4), (-1, 4), (4, 0), (4, -3), (0, 0))] == [-1] * 5
    i = text.index("long long mi_ppo_minibatch_advantages_stats_doubles")
    comment = text[text.rfind("/*", 0, i):i]
    for c in ("PER MINIBATCH", "normalize_advantage", "norm_adv", "No engine handle", "e (T + 1) + t", "slot == T", "does not count", "mean = sum(a) / c",
              "ss = sum((a - mean)^2)", "(c - ddof >= 1) ? sqrt(ss / (c - ddof)) : 0.0", "(float)((a - mean) / (std + 1e-8))", "a true division", "{c, mean, std}",
              "{0, 0, 0}", "torch's .std()", "One launch, one block per minibatch", "read from global memory again", "wave order", "no floating-point atomics",
              "bitwise equal", "neither read", "nor written", "3 ceil(n / batch_size)", "MI_ROLLOUT_MAX_ENVS", "MI_ROLLOUT_MAX_HORIZON", "ddof outside {0, 1}"):
        assert c in comment, c


def test_every_argument_error_before_the_launch():
    """No check needs a device and every one runs before the launch: the dummy host buffers are never written.  Each message names the entry and the argument."""
    from mi355 import lib as milib
    L = milib.get()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    err = L.cdll.mi_last_error
    fn = L.cdll.mi_ppo_minibatch_advantages

    def call(adv_raw=p, perm=p, n=7, batch_size=4, num_envs=3, T=5, ddof=0, tab_adv_out=p, stats=p):
        return fn(None, adv_raw, perm, n, batch_size, num_envs, T, ddof, tab_adv_out, stats)
    me = b"mi_ppo_minibatch_advantages: "
    for name in ("adv_raw", "perm", "tab_adv_out", "stats"):
        assert call(**{name: None}) == -1 and err().startswith(me + name.encode() + b" is missing"), name
    for bad in (0, -1):
        assert call(n=bad) == -1 and err().startswith(me + b"n:"), bad
        assert call(batch_size=bad) == -1 and err().startswith(me + b"batch_size"), bad
    for bad in (0, -2, 1025):
        assert call(num_envs=bad) == -1 and err().startswith(me + b"num_envs outside [1, MI_ROLLOUT_MAX_ENVS]"), bad
    for bad in (0, -1, 4097):
        assert call(T=bad) == -1 and err().startswith(me + b"T outside [1, MI_ROLLOUT_MAX_HORIZON]"), bad
    for bad in (-1, 2, 7):
        assert call(ddof=bad) == -1 and err().startswith(me + b"ddof"), bad
    assert call(num_envs=1024, T=4096, n=2 ** 31 - 1, batch_size=2 ** 31 - 1, ddof=2) == -1 and err().startswith(me + b"ddof")      # the limits are valid: the next check answers
    assert call(n=0, batch_size=0) == -1 and err().startswith(me + b"n:")            # in the order of the argument list
    assert all(x == 0.0 for x in buf)
    with pytest.raises(milib.MiError, match=r"mi_ppo_minibatch_advantages failed \(-1\): mi_ppo_minibatch_advantages: adv_raw is missing"):
        L.mi_ppo_minibatch_advantages(None, None, None, 7, 4, 3, 5, 0, None, None)
    # the neighbours keep their messages
    assert L.cdll.mi_ppo_value_clip_stats(None, p, p, p, p, 8, 0, ctypes.c_float(0.2), 0, p, p) == -1 and err().startswith(b"mi_ppo_value_clip_stats: empty input")
    assert L.cdll.mi_rollout_finish(None, None, p, p, p, 3, 5, ctypes.c_double(0.99), ctypes.c_double(0.95), p, p, None, None, None) == -1
    assert err() == b"mi_rollout_finish: missing buffers"


def test_setting_validation_and_the_off_state_need_no_device():
    from rollout import ContinuousRolloutBuffer, RolloutBuffer, minibatch_normalization_ddof as checked
    assert hasattr(RolloutBuffer, "set_minibatch_normalization")
    assert ContinuousRolloutBuffer.set_minibatch_normalization is RolloutBuffer.set_minibatch_normalization      # one body for both classes
    assert checked() == 0 and checked(1) == 1 and type(checked(np.int64(1))) is int and checked(np.int32(0)) == 0
    for bad in (True, False, np.bool_(True), "0", "1", 0.0, 1.0, np.float64(1.0), 2, -1, [0], (1,), None, float("nan")):
        with pytest.raises(ValueError, match="who: ddof is 0 .population std. or 1"):
            checked(bad, who="who")
    for cls in (RolloutBuffer, ContinuousRolloutBuffer):
        buf = object.__new__(cls)                                                    # as the older host tests build their stubs: no __init__, no attribute
        assert not hasattr(buf, "_minibatch_norm") and getattr(buf, "_minibatch_norm", None) is None
        for bad in (True, "1", 1.0, 2, -1):
            with pytest.raises(ValueError, match="RolloutBuffer.set_minibatch_normalization: ddof is 0"):
                buf.set_minibatch_normalization(bad)
            assert not hasattr(buf, "_minibatch_norm")                               # a refused call changes nothing
        buf.set_minibatch_normalization()
        assert buf._minibatch_norm == {"ddof": 0}
        buf.set_minibatch_normalization(ddof=1)
        assert buf._minibatch_norm == {"ddof": 1}
        buf._minibatch_advantages = "the table"
        with pytest.raises(ValueError):
            buf.set_minibatch_normalization(3)
        assert buf._minibatch_norm == {"ddof": 1} and buf._minibatch_advantages == "the table"
        buf.set_minibatch_normalization(None)
        assert buf._minibatch_norm is None and buf._minibatch_advantages is None     # off, and the table is dropped
    # update() reads the setting so that an object without the attribute means "off"
    assert 'getattr(self, "_minibatch_norm", None)' in inspect.getsource(RolloutBuffer._update)


def test_signatures_and_documents():
    import rollout
    from rollout import ContinuousRolloutBuffer as C, RolloutBuffer as B
    names = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    defaults = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}      # noqa: E731
    assert names(B.set_minibatch_normalization) == ["self", "ddof"] and defaults(B.set_minibatch_normalization) == dict(ddof=0)
    # pinned by the older tests, unchanged here
    assert names(B.update) == ["self", "gamma", "lam", "num_epochs", "batch_size", "stage_times"]
    assert defaults(B.update) == dict(gamma=0.99, lam=0.95, num_epochs=3, batch_size=32, stage_times=None)
    assert names(B.update_with_diagnostics) == names(B.update) + ["target_kl"]
    assert names(C.update) == ["self", "gamma", "lam", "num_epochs", "batch_size", "normalize", "stage_times"]
    assert names(C.update_with_diagnostics) == names(C.update) + ["target_kl"]
    for c in ("set_minibatch_normalization()", "mi_ppo_minibatch_advantages", "minibatch_adv_stats", "minibatch_advantages", "PER MINIBATCH", "normalize_advantage=True",
              "norm_adv=True", "ddof=0 by default", "ddof=1", "one-sample minibatch", "yields 0", "instead of being left unnormalised", "Two deviations from SB3",
              '"minibatch_norm"', "NOT read by the steps"):
        assert c in rollout.__doc__, c
    doc = B.update.__doc__
    for c in ("set_minibatch_normalization", "minibatch_adv_stats", "minibatch_advantages", "did NOT read it", '"minibatch_norm"', '"sgd"'):
        assert c in doc, c
    for rel_path, needles in (("INTEGRATION.md", ("set_minibatch_normalization", "mi_ppo_minibatch_advantages", "minibatch_adv_stats", "ddof=1")),
                              ("DESIGN.md", ("mi_ppo_minibatch_advantages", "ppo_minibatch_adv_kernel")), ("README.md", ("mi_ppo_minibatch_advantages",)),
                              ("profiles/r19_minibatch_advantages.md", ("mi_ppo_minibatch_advantages", "minibatch_norm"))):
        text = open(os.path.join(ROOT, rel_path)).read()
        for c in needles:
            assert c in text, (rel_path, c)


MI = r"_ZN2mi"
NEW_KERNEL = MI + r"24ppo_minibatch_adv_kernelE"
OLD_KERNELS = [MI + r"21rollout_finish_kernelE", MI + r"25rollout_finish_seg_kernelILi0EE", MI + r"25rollout_finish_seg_kernelILi1EE",
               MI + r"30rollout_finish_seg_boot_kernelILi0EE", MI + r"30rollout_finish_seg_boot_kernelILi1EE", MI + r"25rollout_seg_reduce_kernelILi0EE",
               MI + r"25rollout_seg_reduce_kernelILi1EE", MI + r"23rollout_seg_norm_kernelILi0EE", MI + r"23rollout_seg_norm_kernelILi1EE",
               MI + r"26rollout_reward_scan_kernelE", MI + r"25rollout_reward_dev_kernelE", MI + r"27rollout_reward_merge_kernelE", MI + r"27rollout_reward_scale_kernelE",
               MI + r"27ppo_value_clip_stats_kernelE", MI + r"28ppo_value_clip_reduce_kernelE"]


def test_the_new_kernel_in_the_gfx950_listing():
    text = _listing("ppo_ops")
    name = _kernel(text, NEW_KERNEL)[0]
    old = {_kernel(text, prefix)[0] for prefix in OLD_KERNELS}                      # the finish, reward-scaling and value-clipping kernels keep their names
    assert len(old) == len(OLD_KERNELS) and name not in old
