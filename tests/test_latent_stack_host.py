"""Latent stacking, as far as a machine without a GPU can check it: the numpy restatement of tests/latent_stack_cases.py against a hand-written example, the four C
entries, the stacked() constructors, the fresh-flag book-keeping of the step class and both buffers on a stub library, every refusal with its message, the history_state() round
trip, and that latent_stack=1 allocates nothing and calls what was always called."""
import ctypes
import inspect
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "carla-ppo_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import latent_stack_cases as lc  # noqa: E402

NEW = ("mi_rollout_step_batch_stack", "mi_rollout_value_batch_stack", "mi_mlp_rollout_step_batch_stack", "mi_mlp_rollout_value_batch_stack")
STEP_ARGS = ["stream", "frames_u8", "measurements", "n_meas", "noise", "greedy", "n", "scratch", "scratch_bytes", "out", "obs_mean", "obs_inv_std", "obs_clip", "table_rows",
             "n_table_rows", "tab_states", "tab_raw_states", "tab_actions", "tab_values", "latent_stack", "hist", "n_lanes", "lanes", "first", "advance", "sstate", "older_out"]
VALUE_ARGS = ["stream", "frames_u8", "measurements", "n_meas", "n", "scratch", "scratch_bytes", "out", "obs_mean", "obs_inv_std", "obs_clip", "table_rows", "n_table_rows",
              "tab_final_values", "latent_stack", "hist", "n_lanes", "lanes", "first", "sstate"]


# ---- 1: the restatement against an example written out by hand ----
def test_restatement_against_a_hand_written_example():
    """3 lanes, k = 3, z_dim = 2, one measurement, five calls.  Latent of lane l at its j-th step: [10 l + j, -(10 l + j)]; written below as the scalar 10 l + j."""
    def z(*v):
        return np.array([[x, -x] for x in v], np.float32)

    def row(cur, o1, o2, m):
        return [cur, -cur, o1, -o1, o2, -o2, m]
    h = lc.HostStack(3, 3, 2)
    # call 1: all lanes, all fresh: every row repeats its own latent
    r = h.call([0, 1, 2], z(1, 11, 21), [[0.5], [1.5], [2.5]])
    assert r.tolist() == [row(1, 1, 1, 0.5), row(11, 11, 11, 1.5), row(21, 21, 21, 2.5)]
    assert h.hist.tolist() == [[[1, -1], [1, -1]], [[11, -11], [11, -11]], [[21, -21], [21, -21]]]
    # call 2: lanes [2, 0] in that order; lane 1 is skipped and keeps its history
    r = h.call([2, 0], z(22, 2), [[7.0], [8.0]])
    assert r.tolist() == [row(22, 21, 21, 7.0), row(2, 1, 1, 8.0)]
    assert h.hist.tolist() == [[[2, -2], [1, -1]], [[11, -11], [11, -11]], [[22, -22], [21, -21]]]
    # lane 0 restarts; call 3: all lanes
    h.restart([0])
    r = h.call([0, 1, 2], z(3, 12, 23), [[0.0], [0.0], [0.0]])
    assert r.tolist() == [row(3, 3, 3, 0.0), row(12, 11, 11, 0.0), row(23, 22, 21, 0.0)]
    assert h.hist.tolist() == [[[3, -3], [3, -3]], [[12, -12], [11, -11]], [[23, -23], [22, -22]]]
    # call 4: advance = False (a bootstrap): the rows are assembled, nothing moves, nobody stops being fresh
    h.restart([1])
    before, fresh = h.hist.copy(), h.fresh.copy()
    r = h.call([1, 2], z(13, 24), [[1.0], [2.0]], advance=False)
    assert r.tolist() == [row(13, 13, 13, 1.0), row(24, 23, 22, 2.0)]
    assert np.array_equal(h.hist, before) and np.array_equal(h.fresh, fresh) and fresh.tolist() == [False, True, False]
    # call 5: the same observations stepped again
    r = h.call([1, 2], z(13, 24), [[1.0], [2.0]])
    assert r.tolist() == [row(13, 13, 13, 1.0), row(24, 23, 22, 2.0)]
    assert h.hist.tolist() == [[[3, -3], [3, -3]], [[13, -13], [13, -13]], [[24, -24], [23, -23]]] and not h.fresh.any()


def test_restatement_select_and_lanes_outside_the_history():
    """NaN in a history that `first` overrides does not reach the row; a lane outside [0, n_lanes) is `first` and nothing of the history changes for it; k = 2 has
    nothing to move: the new history is the latent."""
    hist = np.full((2, 1, 3), np.nan, np.float32)
    z = np.arange(6, dtype=np.float32).reshape(2, 3)
    rows = lc.stack_rows(hist, [1, 5], [1, 0], z, np.zeros((2, 0)))
    assert rows.tolist() == [[0, 1, 2, 0, 1, 2], [3, 4, 5, 3, 4, 5]]
    new = lc.shift(hist, [1, 5], [1, 0], z)
    assert np.isnan(new[0]).all() and new[1].tolist() == [[0, 1, 2]]
    rows = lc.stack_rows(hist, [0], [0], z[:1], [[9.0]])                             # not first: the NaN is the history and is copied
    assert np.isnan(rows[0, 3:6]).all() and rows[0, 6] == 9.0
    for zd, k, nm in lc.KERNEL_SHAPES:
        assert 2 <= k <= 16 and lc.din_of(zd, k, nm) <= 1024
    assert sorted(lc.din_of(*s) for s in lc.KERNEL_SHAPES) == [19, 29, 127, 128, 129, 259, 1024]


# ---- the C entries and the keywords ----
def test_the_four_entries_are_exported_with_the_headers_prototypes():
    from mi355 import lib as milib
    L = milib.get()
    protos = milib.parse_header()
    for name in NEW:
        assert name in protos and hasattr(L.cdll, name), name
        ret, args = protos[name]
        assert ret == "int" and [a[1] for a in args][2:] == (VALUE_ARGS if "value" in name else STEP_ARGS), name
    assert [a[0] for a in protos["mi_rollout_step_batch_stack"][1]] == [a[0] for a in protos["mi_mlp_rollout_step_batch_stack"][1]]
    assert [a[0] for a in protos["mi_rollout_value_batch_stack"][1]] == [a[0] for a in protos["mi_mlp_rollout_value_batch_stack"][1]]
    text = open(milib.HEADER).read()
    assert "#define MI_ROLLOUT_MAX_STACK 16" in text
    import rollout
    assert rollout.MAX_STACK == 16 and rollout.MAX_STACK_INPUTS == 1024
    assert L.mi_abi_version() == 7


def test_the_stacked_constructors_and_the_pinned_signatures():
    """Stacking is reached through a classmethod of each class and BatchedRolloutStep.step(); the constructors and __call__ keep the signatures they had."""
    import rollout
    sig = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert sig(rollout.BatchedRolloutStep.stacked) == ["vae", "ppo", "num_envs", "latent_stack", "seed", "io"]
    assert sig(rollout.RolloutStep.stacked) == ["vae", "ppo", "latent_stack", "seed", "io"]
    for cls in (rollout.RolloutBuffer, rollout.ContinuousRolloutBuffer):
        assert sig(cls.stacked) == ["vae", "ppo", "num_envs", "horizon", "latent_stack", "seed", "io"], cls
        assert sig(cls.__init__) == ["self", "vae", "ppo", "num_envs", "horizon", "seed", "io"], cls
    assert sig(rollout.BatchedRolloutStep.__init__) == ["self", "vae", "ppo", "num_envs", "seed", "io"]
    assert sig(rollout.BatchedRolloutStep.__call__) == ["self", "frames_u8", "measurements", "greedy", "noise"]
    p = inspect.signature(rollout.BatchedRolloutStep.step).parameters
    assert list(p) == ["self", "frames_u8", "measurements", "env_ids", "greedy", "noise"] and p["env_ids"].default is None
    assert list(p) == sig(rollout.RolloutBuffer.step)
    for name in ("restart_history", "history_state", "load_history_state"):
        assert hasattr(rollout.RolloutBuffer, name), name
    for name in ("restart", "history_state", "load_history_state"):
        assert hasattr(rollout.BatchedRolloutStep, name), name
    doc = " ".join(rollout.__doc__.split())                                          # (however the paragraph is wrapped)
    assert "latent_stack=4" in doc and "ppo.set_wide_inputs()" in doc and "With the setting off no tensor is allocated and every call makes the launches it always made" in doc


def test_c_argument_errors_before_any_launch():
    """latent_stack outside 2 .. 16 and a NULL hist, lanes, first or sstate come back before a handle is read: the dummy host buffers are never written."""
    from mi355 import lib as milib
    L = milib.get()
    buf = (ctypes.c_double * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    err = L.cdll.mi_last_error
    flt = ctypes.c_float

    def step(entry, k=4, hist=p, n_lanes=4, lanes=p, first=p, sstate=p, mean=None, inv=None, clip=0.0, rows=None, ts=None, tr=None, h=p):
        return getattr(L.cdll, entry)(h, p, None, p, p, 3, None, 1, 4, p, ctypes.c_longlong(0), p, mean, inv, flt(clip), rows, ctypes.c_longlong(8), ts, tr, p, p, k, hist, n_lanes,
                                      lanes, first, 1, sstate, p)

    def value(entry, k=4, hist=p, n_lanes=4, lanes=p, first=p, sstate=p, mean=None, inv=None, clip=0.0, h=p):
        return getattr(L.cdll, entry)(h, p, None, p, p, 3, 4, p, ctypes.c_longlong(0), p, mean, inv, flt(clip), p, ctypes.c_longlong(8), p, k, hist, n_lanes, lanes, first, sstate)
    for entry in NEW:
        call = value if "value" in entry else step
        me = entry.encode() + b": "
        assert call(entry, h=None) == -4 and err() == me + b"null handle"
        for k in (1, 0, -3, 17):
            assert call(entry, k=k) == -1 and err() == me + b"2 <= latent_stack <= MI_ROLLOUT_MAX_STACK", (entry, k)
        for kw in (dict(hist=None), dict(lanes=None), dict(first=None), dict(sstate=None), dict(n_lanes=0)):
            assert call(entry, **kw) == -1 and err() == me + b"missing hist / lanes / first / sstate", (entry, kw)
        assert call(entry, sstate=odd) == -1 and err() == me + b"sstate must be 16-byte aligned"
        for bad in (0.0, -1.0, float("nan")):
            assert call(entry, mean=p, inv=p, clip=bad) == -1 and err().startswith(me + b"obs_inv_std is missing or obs_clip"), (entry, bad)
        assert call(entry, mean=p, inv=None, clip=1.0) == -1 and err().startswith(me + b"obs_inv_std is missing")
        assert call(entry, inv=p) == -1 and err().startswith(me + b"obs_inv_std and tab_raw_states are NULL where obs_mean is")
    for entry in (NEW[0], NEW[2]):
        me = entry.encode() + b": "
        assert step(entry, rows=p, ts=None) == -1 and err() == me + b"missing tables"
        assert step(entry, rows=p, ts=p, mean=p, inv=p, clip=1.0, tr=None) == -1 and err() == me + b"missing tables"
        assert step(entry, tr=p) == -1 and err().startswith(me + b"obs_inv_std and tab_raw_states are NULL where obs_mean is")
    assert all(x == 0.0 for x in buf)
    # the neighbours keep their messages
    assert L.cdll.mi_rollout_step_batch(p, p, None, None, p, 3, None, 1, 4, p, 0, p) == -1 and err() == b"mi_rollout_step_batch: missing buffers"
    assert L.cdll.mi_rollout_step_batch_rec(p, p, None, p, p, 3, None, 1, 4, p, 0, p, p, 8, None, p, p) == -1 and err() == b"mi_rollout_step_batch_rec: missing tables"


# ---- a stub library, fake engines, CPU tensors in place of the pinned / device ones ----
class StubLib:
    def __init__(self):
        self.calls = []
        self.cdll = types.SimpleNamespace(mi_last_error=lambda: b"")

    def __getattr__(self, name):
        if not name.startswith("mi_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, len(args), args))
            return 64 if name.endswith("_workspace_bytes") else 0
        return entry


class FakeDev:
    source_shape = (2, 2, 3)
    device = "cpu"
    handle = 1

    def __init__(self, kind, lib):
        self.L = lib
        if kind is not None:
            self.rollout_kind = kind

    def ensure_batch(self, n):
        pass

    def _desc(self, n):
        return ctypes.c_int(0)


class FakeModel:
    seed = 0

    def __init__(self, z_dim=4, input_dim=7, num_actions=2, kind=None, lib=None):
        self.z_dim, self.input_dim, self.num_actions = z_dim, input_dim, num_actions
        self.dev = FakeDev(kind, lib if lib is not None else StubLib())

    def _need_dev(self):
        return self.dev


@pytest.fixture
def cpu(monkeypatch):
    """The real constructors on CPU tensors: no pinning, a stream that does nothing."""
    import torch
    import rollout

    def io(self, in_bytes, out_floats):
        self.h_in, self.h_out = torch.zeros(in_bytes, dtype=torch.uint8), torch.zeros(out_floats)
        self.d_in = self.d_out = None
        self._in_np = self.h_in.numpy()
    monkeypatch.setattr(rollout._StepBase, "_io_buffers", io)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0, synchronize=lambda: None))
    return rollout


def models(k, kind=None, z=4, n_meas=3):
    lib = StubLib()
    return FakeModel(z, k * z + n_meas, kind=kind, lib=lib), FakeModel(z, k * z + n_meas, lib=lib), lib


def obs(n, n_meas=3):
    return np.zeros((n, 2, 2, 3), np.uint8), np.zeros((n, n_meas))


# ---- 2: the fresh flags ----
def test_step_class_lanes_flags_and_arguments(cpu):
    vae, ppo, lib = models(3)
    s = cpu.BatchedRolloutStep.stacked(vae, ppo, 4, 3)
    assert s.k == 3 and s.n_meas == 3 and s.din == 15 and s.latent_cols == 12
    assert tuple(s.history.shape) == (4, 2, 4) and float(s.history.abs().sum()) == 0.0 and s.fresh.tolist() == [True] * 4 and tuple(s.sstate.shape) == (4, 15)
    assert s.h_in.numel() == s._f_off + 4 * 4 * (3 + 2 + 0 + 2) and s.h_out.numel() == 4 * (2 + 1 + 4) + 4 * 2 * 4
    del lib.calls[:]
    a, v, states = s(*obs(4))
    assert states.shape == (4, 15) and states.dtype == np.float64 and not s.fresh.any()
    name, count, args = lib.calls[-1]
    assert (name, count) == ("mi_rollout_step_batch_stack", 29)
    fptr = s.h_in.data_ptr() + s._f_off
    assert args[12:15] == (None, None, 0.0) and args[15:21] == (None, 0, None, None, None, None)
    assert args[21:] == (3, s.history.data_ptr(), 4, fptr + 4 * (12 + 8), fptr + 4 * (12 + 8 + 4), 1, s.sstate.data_ptr(), s.h_out.data_ptr() + 4 * 4 * 7)
    assert s._i_np[20:24].tolist() == [0, 1, 2, 3] and s._i_np[24:28].tolist() == [1, 1, 1, 1]
    # a subset, in its own order: only these stop being fresh; the flags travel behind the lanes
    s.restart()
    assert s.fresh.all()
    s.step(*obs(2), env_ids=[3, 1])
    assert s.fresh.tolist() == [True, False, True, False]
    assert s._i_np[6 + 4:6 + 4 + 2].tolist() == [3, 1] and s._i_np[6 + 4 + 2:6 + 4 + 4].tolist() == [1, 1]
    s.step(*obs(3), env_ids=[1, 0, 3], greedy=True)
    assert s._i_np[9 + 6 + 3:9 + 6 + 6].tolist() == [0, 1, 0] and not s.fresh[[0, 1, 3]].any() and s.fresh[2]
    s.restart([1])
    assert s.fresh.tolist() == [False, True, True, False]
    for bad, msg in (([0, 0], "duplicate env_ids"), ([0, 4], r"env_ids outside \[0, 4\)"), ([-1, 0], "env_ids outside"), ([0], "env_ids must be a vector of 2 integers"), ([0.0, 1.0], "env_ids must be a vector of 2 integers")):
        with pytest.raises(ValueError, match="BatchedRolloutStep: " + msg):
            s.step(*obs(2), env_ids=bad)
    assert s.fresh.tolist() == [False, True, True, False]
    # an MlpVAE goes to its own entry
    vae, ppo, lib = models(2, kind="mlp")
    s = cpu.BatchedRolloutStep.stacked(vae, ppo, 2, 2)
    s(*obs(2))
    assert lib.calls[-1][:2] == ("mi_mlp_rollout_step_batch_stack", 29)


@pytest.mark.parametrize("continuous", [False, True], ids=["RolloutBuffer", "ContinuousRolloutBuffer"])
def test_buffer_flags(cpu, continuous):
    vae, ppo, lib = models(2)
    E, T = 3, 4
    b = (cpu.ContinuousRolloutBuffer if continuous else cpu.RolloutBuffer).stacked(vae, ppo, E, T, 2)
    s = b._step
    assert b.history is s.history and tuple(b.history.shape) == (E, 1, 4) and tuple(b.states.shape) == (E * (T + 1), 11)
    b.reset()
    assert s.fresh.all()
    b.step(*obs(E))
    assert lib.calls[-1][:2] == ("mi_rollout_step_batch_stack", 29) and lib.calls[-1][2][26] == 1 and not s.fresh.any()
    assert lib.calls[-1][2][16] == b.n_table_rows and lib.calls[-1][2][17] == b.states.data_ptr() and lib.calls[-1][2][18] is None
    b.outcome(np.zeros(E), np.array([False, True, False]))                           # done: fresh for its next step
    assert s.fresh.tolist() == [False, True, False]
    if continuous:
        b.step(*obs(E))
        assert not s.fresh.any()
        b.outcome(np.zeros(E), np.zeros(E, bool))
        b.truncate(*obs(1), env_ids=[2])                                             # valued on the running history, then fresh
        name, count, args = lib.calls[-1]
        assert (name, count) == ("mi_rollout_value_batch_stack", 22) and args[16:19] == (2, s.history.data_ptr(), E)
        assert s._i_np[3 + 1:3 + 3].tolist() == [2, 0] and s.fresh.tolist() == [False, False, True]
        b.step(*obs(2), env_ids=[0, 2])                                              # a subset of the lanes
        assert s.fresh.tolist() == [False, False, False]
        b.outcome(np.zeros(2), np.array([False, True]), env_ids=[0, 2])
        assert s.fresh.tolist() == [False, False, True]
        need = b.rows.needs_bootstrap()
    else:
        b.step(*obs(2), env_ids=[2, 0])
        b.outcome(np.zeros(2), np.array([True, False]), env_ids=[2, 0])
        assert s.fresh.tolist() == [False, True, True]
        need = b.rows.stepped()
    flags = s.fresh.copy()
    b.bootstrap(*obs(len(need)), env_ids=need)                                       # a recording call that advances nothing
    name, count, args = lib.calls[-1]
    assert (name, count) == ("mi_rollout_step_batch_stack", 29) and args[26] == 0 and args[7] == 1 and np.array_equal(s.fresh, flags)
    b.reset()                                                                        # an episode may continue across an update
    assert np.array_equal(s.fresh, flags)
    b.restart_history([0])
    assert s.fresh[0] and np.array_equal(s.fresh[1:], flags[1:])
    b.restart_history()
    assert s.fresh.all()
    for bad in ([0, 0], [3], [[0]]):
        with pytest.raises(ValueError, match="RolloutBuffer: "):
            b.restart_history(bad)


def test_observation_normalisation_counts_the_stacked_latents(cpu):
    """normalize_latents=False spares the first k z_dim columns, the state keeps k z_dim as its z_dim, and a state of another split is refused."""
    vae, ppo, lib = models(3)
    b = cpu.RolloutBuffer.stacked(vae, ppo, 2, 3, 3)
    b.set_observation_normalization(normalize_latents=False)
    name, _, args = lib.calls[-1]
    assert name == "mi_rollout_obs_stats" and args[5] == 15 and args[6] == 12
    sd = b.observation_normalization_state()
    assert sd["z_dim"] == 12 and sd["mean"].shape == (15,)
    b.load_observation_normalization_state(sd)
    with pytest.raises(ValueError, match="z_dim = 4, this buffer has 12"):
        b.load_observation_normalization_state(dict(sd, z_dim=4))
    b.reset()
    b.step(*obs(2))
    name, count, args = lib.calls[-1]
    on = b._obs_norm
    assert (name, count) == ("mi_rollout_step_batch_stack", 29) and args[12:15] == (on["mean32"].data_ptr(), on["inv32"].data_ptr(), on["clip"])
    assert args[17] == b.states.data_ptr() and args[18] == b.raw_states.data_ptr()
    s = cpu.BatchedRolloutStep.stacked(vae, ppo, 2, 3)
    s.set_observation_normalization(sd)
    with pytest.raises(ValueError, match="z_dim = 4, this step has 12"):
        s.set_observation_normalization(dict(sd, z_dim=4))


# ---- 3: the refusals of the Python side ----
def test_python_refusals_before_anything_touches_a_device(cpu):
    import rollout

    class NoDevice(FakeModel):
        def _need_dev(self):
            raise AssertionError("a device was asked for")
    vae, ppo = NoDevice(4, 7), NoDevice(4, 7)
    for bad in (0, -1, 17, 2.0, "2", None, True, [2]):
        for make in (lambda k: rollout.BatchedRolloutStep.stacked(vae, ppo, 2, k), lambda k: rollout.RolloutBuffer.stacked(vae, ppo, 2, 3, k),
                     lambda k: rollout.ContinuousRolloutBuffer.stacked(vae, ppo, 2, 3, k)):
            with pytest.raises(ValueError, match=r"latent_stack is an int in \[1, 16\]"):
                make(bad)
    with pytest.raises(ValueError, match=r"BatchedRolloutStep: latent_stack = 2 latents of 4 are 8 inputs, the policy takes 7"):
        rollout.BatchedRolloutStep.stacked(vae, ppo, 2, 2)
    with pytest.raises(ValueError, match=r"RolloutBuffer: latent_stack = 2 latents of 4 are 8 inputs, the policy takes 7"):
        rollout.RolloutBuffer.stacked(vae, ppo, 2, 3, 2)
    with pytest.raises(ValueError, match="fewer inputs than the VAE's latent size"):      # latent_stack = 1: the message it always was
        rollout.BatchedRolloutStep(NoDevice(8, 7), NoDevice(8, 7), 2)
    wide_v, wide_p = NoDevice(64, 16 * 64 + 1), NoDevice(64, 16 * 64 + 1)
    with pytest.raises(ValueError, match=r"latent_stack = 16 gives a state of 1025 inputs, the stacked step assembles at most 1024"):
        rollout.ContinuousRolloutBuffer.stacked(wide_v, wide_p, 2, 3, 16)
    with pytest.raises(ValueError, match=r"latent_stack = 2 gives a state of 1025 inputs"):
        rollout.BatchedRolloutStep.stacked(wide_v, wide_p, 2, 2)
    for bad in (2, 0, None, 1.0, True):
        with pytest.raises(ValueError, match=r"RolloutStep: latent stacking .*BatchedRolloutStep\.stacked\(vae, ppo, num_envs=1, latent_stack=k\)"):
            rollout.RolloutStep.stacked(vae, ppo, bad)
    # with the setting off: what belongs to it says so
    vae, ppo, lib = models(1)
    s = rollout.BatchedRolloutStep(vae, ppo, 2)
    for call in (s.restart, s.history_state, lambda: s.load_history_state({})):
        with pytest.raises(ValueError, match=r"latent stacking is off \(build it with stacked"):
            call()


# ---- 4: the state round trip ----
def test_history_state_round_trip_and_refusals(cpu):
    import torch
    vae, ppo, lib = models(3)
    a = cpu.RolloutBuffer.stacked(vae, ppo, 3, 4, 3)
    a.history.copy_(torch.arange(24, dtype=torch.float32).reshape(3, 2, 4))
    a._step.fresh[:] = [False, True, False]
    d = a.history_state()
    assert set(d) == {"latent_stack", "z_dim", "history", "fresh"} and d["latent_stack"] == 3 and d["z_dim"] == 4
    assert d["history"].dtype == np.float32 and d["history"].shape == (3, 2, 4) and d["fresh"].tolist() == [False, True, False]
    b = cpu.ContinuousRolloutBuffer.stacked(vae, ppo, 3, 4, 3)
    b.load_history_state(d)
    assert torch.equal(b.history, a.history) and b._step.fresh.tolist() == [False, True, False]
    d["fresh"][0] = True                                                             # a copy: the buffer's own flags do not follow
    assert not a._step.fresh[0] and not b._step.fresh[0]
    good = b.history_state()
    hist, fresh = b.history.clone(), b._step.fresh.copy()
    bads = [dict(good, latent_stack=2), dict(good, latent_stack=3.0), dict(good, z_dim=8), dict(good, history=good["history"][:2]), dict(good, history=good["history"][:, :1]),
            dict(good, history=good["history"].astype(np.int32)), dict(good, fresh=good["fresh"][:2]), dict(good, fresh=good["fresh"].astype(np.int32)),
            {k: v for k, v in good.items() if k != "fresh"}, {k: v for k, v in good.items() if k != "history"}, {k: v for k, v in good.items() if k != "z_dim"}, None, []]
    for bad in bads:
        with pytest.raises(ValueError, match="RolloutBuffer.load_history_state: "):
            b.load_history_state(bad)
        assert torch.equal(b.history, hist) and np.array_equal(b._step.fresh, fresh)
    with pytest.raises(ValueError, match="latent_stack = 2, this one has 3"):
        b.load_history_state(dict(good, latent_stack=2))
    with pytest.raises(ValueError, match="expected a dict with the keys latent_stack, z_dim, history, fresh"):
        b.load_history_state({k: v for k, v in good.items() if k != "fresh"})


# ---- 5: the setting off ----
@pytest.mark.parametrize("kind", [None, "mlp"])
def test_latent_stack_one_allocates_nothing_and_calls_what_was_always_called(cpu, kind):
    vae, ppo, lib = models(1, kind=kind)
    b = cpu.ContinuousRolloutBuffer(vae, ppo, 3, 4)
    s = b._step
    assert s.k == 1 and b.history is None and not hasattr(s, "history") and not hasattr(s, "fresh") and not hasattr(s, "sstate")
    assert s.h_in.numel() == s._f_off + 4 * 3 * (3 + 2 + 1) and s.h_out.numel() == 3 * 7
    frames, meas = obs(3)
    b.reset()
    b.step(frames, meas)
    b.outcome(np.zeros(3), np.array([False, True, False]))
    b.truncate(frames[:1], meas[:1], env_ids=[0])
    b.bootstrap(frames[2:], meas[2:], env_ids=[2])
    plain = cpu.BatchedRolloutStep(vae, ppo, 2)
    a, v, states = plain.step(frames[:2], meas[:2], greedy=True, env_ids=[1, 0])          # env_ids is checked and not used
    assert states.shape == (2, 7)
    with pytest.raises(ValueError, match="duplicate env_ids"):
        plain.step(frames[:2], meas[:2], env_ids=[1, 1])
    got = [c[:2] for c in lib.calls if "rollout" in c[0] and "workspace" not in c[0]]
    if kind == "mlp":
        assert got == [("mi_mlp_rollout_step_batch", 22), ("mi_mlp_rollout_value_batch", 17), ("mi_mlp_rollout_step_batch", 22), ("mi_mlp_rollout_step_batch", 22)]
    else:
        assert got == [("mi_rollout_step_batch_rec", 17), ("mi_rollout_value_batch_rec", 13), ("mi_rollout_step_batch_rec", 17), ("mi_rollout_step_batch", 12)]
    assert not any("stack" in c[0] for c in lib.calls)
